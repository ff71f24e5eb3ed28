"""ENet's x2-upsample StyleConv as nine 1x1 tap products and one bilinear tap-sum pass (ops.tapsum_up2,
engine/enet.py TAPSUM).  Bilinear upsampling is linear and per channel, so it commutes with a 1x1 channel mix:

    conv3x3(up2(x))[r, c] = sum over taps t = (dy, dx) of up2(W_t x)[r + dy - 1, c + dx - 1]   (zero outside the frame)

The tap-sum alone against fp64 on every output pixel, windows against the whole frame bit for bit, the composed
layer against the reference order (upsample, then the per-sample 3x3 conv) on the whole frame, the premodulated
tap-product weights against the in-launch modulation, and the engine with the switch on against off."""
import math

import pytest
import torch
import torch.nn.functional as F

import s2v_import  # noqa: F401
from s2v_amd import ops, synth
from s2v_amd.engine import enet as E
from s2v_amd.ops import NHWC, ConvW

DEV = "cuda"
pytestmark = pytest.mark.gpu

# per-product bounds of the conv arithmetic modes and ENet's output bound in f16x3, restated from
# tests/test_ops_gpu.py (REL) and tests/test_models_gpu.py (TOL["f16x3"]["enet"])
REL = {"f32": 2e-6, "bf16x3": 5e-5, "f16x3": 3e-6}
ENET_TOL_F16X3 = (6e-4, 6e-5)


@pytest.fixture(scope="module")
def ctx():
    return ops.Ctx(DEV)


def rnd(*shape, seed=0, lo=-1.0, hi=1.0):
    g = torch.Generator().manual_seed(seed)
    return lo + (hi - lo) * torch.rand(*shape, generator=g, dtype=torch.float64)


def dev32(t):
    return t.float().contiguous().to(DEV)


def tapsum_fp64(p, cout, noise=None, pix_w=0.0, bias=None, lrelu=None):
    """fp64 reference of ops.tapsum_up2 on the whole frame: p [n, h, w, 9 cout] (tap-major) -> (y, bound), both
    [n, 2h, 2w, cout]; bound = sum |coefficient * P| + |noise term| + |bias|."""
    n, h, w, _ = p.shape

    def taps(q):
        up = F.interpolate(q.permute(0, 3, 1, 2), scale_factor=2, mode="bilinear", align_corners=False)
        up = F.pad(up.reshape(n, 9, cout, 2 * h, 2 * w), (1, 1, 1, 1))
        return sum(up[:, 3 * dy + dx, :, dy: dy + 2 * h, dx: dx + 2 * w] for dy in range(3) for dx in range(3))
    y, bound = taps(p), taps(p.abs())
    if bias is not None:
        y = y + bias[None, :, None, None]
        bound = bound + bias.abs()[None, :, None, None]
    if noise is not None:
        y = y + pix_w * noise[:, None]
        bound = bound + (pix_w * noise).abs()[:, None]
    if lrelu is not None:
        y = F.leaky_relu(y, lrelu)
    return y.permute(0, 2, 3, 1), bound.permute(0, 2, 3, 1)


@pytest.mark.parametrize("extras", [False, True])
@pytest.mark.parametrize("h,w", [(5, 7), (1, 3)])
def test_tapsum_up2_against_fp64(ctx, h, w, extras):
    """y = act(sum_t bil(P_t)(r + dy - 1, c + dx - 1) + bias + pix_w noise) against fp64 built from F.interpolate,
    F.pad and nine shifted adds, on every output pixel (the frame's outermost lines included; h = 1: every row
    clamped).  Bound per element: 2^-18 (sum |coefficient P| + |noise term| + |bias|) + 1e-7, i.e. 36 fp32 FMAs at
    2^-24 each with a x4 margin."""
    n, cout = 2, 8
    p = rnd(n, h, w, 9 * cout, seed=1).float().double()
    noise = rnd(n, 2 * h, 2 * w, seed=2).float().double() if extras else None
    bias = rnd(cout, seed=3).float().double() if extras else None
    y = NHWC.empty(n, 2 * h, 2 * w, cout, DEV)
    ops.tapsum_up2(ctx, NHWC(dev32(p)), y, bias=None if bias is None else dev32(bias),
                   pix_add=None if noise is None else dev32(noise), pix_w=0.3 if extras else 0.0,
                   act=ops.ACT_LRELU if extras else ops.ACT_NONE, alpha=0.2)
    ref, bound = tapsum_fp64(p, cout, noise, 0.3, bias, 0.2 if extras else None)
    err = (y.t.cpu().double() - ref).abs()
    tol = 2.0 ** -18 * bound + 1e-7
    print(f"tapsum {h}x{w} extras={extras}: max err {err.max():.3e}, max err / tol {(err / tol).max():.3f}")
    assert (err <= tol).all(), f"max err / tol {(err / tol).max():.3f}"


def test_tapsum_up2_refuses_cout_not_multiple_of_4(ctx):
    n, h, w, cout = 1, 4, 4, 6
    with pytest.raises(Exception, match="multiple of 4"):
        ops.tapsum_up2(ctx, NHWC(dev32(rnd(n, h, w, 9 * cout, seed=1))), NHWC.empty(n, 2 * h, 2 * w, cout, DEV))


@pytest.fixture(scope="module")
def frame12(ctx):
    """The 12 x 12 low-resolution frame with Cout = 32 and its whole-frame tap-sum (computed once)."""
    n, f, cout = 2, 12, 32
    p = dev32(rnd(n, f, f, 9 * cout, seed=11))
    noise = dev32(rnd(n, 2 * f, 2 * f, seed=12))
    bias = dev32(rnd(cout, seed=13))
    full = NHWC.empty(n, 2 * f, 2 * f, cout, DEV)
    ops.tapsum_up2(ctx, NHWC(p), full, bias=bias, pix_add=noise, pix_w=0.1, act=ops.ACT_LRELU, alpha=0.2)
    torch.cuda.synchronize()
    return p, noise, bias, full.t.clone()


def _window_call(ctx, frame12, origin, size, src_origin=None, src_size=None):
    p, noise, bias, _ = frame12
    n, f, cout = p.shape[0], p.shape[1], bias.shape[0]
    (oy, ox), (oh, ow) = origin, size
    (sy, ph), (sx, pw) = ops.up2_tap_window(oy, oh, f), ops.up2_tap_window(ox, ow, f)
    if src_origin is not None:
        (sy, sx), (ph, pw) = src_origin, src_size
    got = NHWC.empty(n, oh, ow, cout, DEV)
    ops.tapsum_up2(ctx, NHWC(p[:, sy: sy + ph, sx: sx + pw].contiguous()), got, bias=bias,
                   pix_add=noise[:, oy: oy + oh, ox: ox + ow].contiguous(), pix_w=0.1, act=ops.ACT_LRELU, alpha=0.2,
                   frame=(f, f), origin=origin, src_origin=(sy, sx))
    torch.cuda.synchronize()
    return got.t, (sy, sx, ph, pw)


# (output window origin, size) in the 24 x 24 frame: the second has 21 x 17 = 357 pixels (no multiple of the block)
# and odd origins (cells half outside the window); the third reads a tap-product window that is not the frame
WINDOWS = [((2, 2), (20, 20)), ((1, 3), (21, 17)), ((6, 4), (10, 12))]


@pytest.mark.parametrize("origin,size", WINDOWS)
def test_tapsum_up2_window_equals_full_frame(ctx, frame12, origin, size):
    """A window call (frame=, origin=, src_origin=) over the tap-product window its taps need against the
    whole-frame call sliced to the window: torch.equal."""
    got, src = _window_call(ctx, frame12, origin, size)
    (oy, ox), (oh, ow) = origin, size
    if origin == (6, 4):
        assert src == (2, 1, 7, 8)              # rows 2..8, columns 1..8 of the 12 x 12 frame
    assert torch.equal(got, frame12[3][:, oy: oy + oh, ox: ox + ow])


def test_tapsum_up2_refuses_a_window_past_the_taps(ctx, frame12):
    """An output window whose taps leave the tap-product window is an error, not an out-of-bounds read."""
    with pytest.raises(Exception, match="outside the 6x8 tap-product window"):   # rows 6..15 read rows 2..8
        _window_call(ctx, frame12, (6, 4), (10, 12), src_origin=(3, 1), src_size=(6, 8))
    with pytest.raises(Exception, match="outside the 7x7 tap-product window"):   # columns 4..15 read columns 1..8
        _window_call(ctx, frame12, (6, 4), (10, 12), src_origin=(2, 1), src_size=(7, 7))
    with pytest.raises(Exception, match="leaves the 24x24 frame"):
        ops.tapsum_up2(ctx, NHWC(frame12[0]), NHWC.empty(2, 20, 12, 32, DEV), frame=(12, 12), origin=(6, 4))


def _layer(n, cin, h, w, cout):
    """The data of tests/test_ops_gpu.py::test_modulated_conv_d2s_polyphase and the tap-product weights."""
    wt = rnd(cout, cin, 3, 3, seed=71) / math.sqrt(cin * 9)
    bias = rnd(cout, seed=72)
    x = rnd(n, cin, h, w, seed=73)
    s = rnd(n, cin, seed=74, lo=0.5, hi=1.5)
    d = rnd(n, cout, seed=75, lo=0.5, hi=1.5)
    noise = rnd(n, 2 * h, 2 * w, seed=76)
    # row t * cout + o = W[o, :, dy, dx], t = 3 dy + dx
    cw9 = ConvW(wt.float().permute(2, 3, 0, 1).reshape(9 * cout, cin, 1, 1), None, DEV)
    return wt, bias, x, s, d, noise, cw9


@pytest.mark.parametrize("n,cin,h,w,cout", [(2, 64, 9, 7, 32), (3, 32, 12, 16, 128)])
def test_tap_product_styleconv_against_reference_order(ctx, prec, n, cin, h, w, cout):
    """The composed layer (modulated 1x1 conv to 9 cout tap products, then the tap-sum with noise + bias +
    LeakyReLU) against the reference order (F.interpolate, then the per-sample 3x3 conv + noise + bias + LeakyReLU,
    base_blocks.py:500-533): the oracle and bound of test_modulated_conv_d2s_polyphase, on the whole frame."""
    wt, bias, x, s, d, noise, cw9 = _layer(n, cin, h, w, cout)
    p = NHWC.empty(n, h, w, 9 * cout, DEV)
    ops.modulated_conv2d(ctx, NHWC(dev32(x.permute(0, 2, 3, 1))), cw9, p, dev32(s), dev32(d.repeat(1, 9)))
    y = NHWC.empty(n, 2 * h, 2 * w, cout, DEV)
    ops.tapsum_up2(ctx, p, y, bias=dev32(bias), pix_add=dev32(noise), pix_w=0.3, act=ops.ACT_LRELU, alpha=0.2)
    up = F.interpolate(x, scale_factor=2, mode="bilinear", align_corners=False)
    wb = wt[None] * s[:, None, :, None, None] * d[:, :, None, None, None]
    conv = torch.stack([F.conv2d(up[i:i + 1], wb[i], bias, padding=1)[0] for i in range(n)])
    ref = F.leaky_relu(conv + 0.3 * noise[:, None], 0.2)
    bound = torch.stack([F.conv2d(up[i:i + 1].abs(), wb[i].abs(), padding=1)[0] for i in range(n)]) + 1
    err = (y.t.cpu().double().permute(0, 3, 1, 2) - ref).abs()
    print(f"tap-product layer {prec} {(n, cin, h, w, cout)}: max err {err.max():.3e}, "
          f"max err / tol {(err / (4 * REL[prec] * bound + 1e-6)).max():.3f}")
    assert (err <= 4 * REL[prec] * bound + 1e-6).all(), f"max err {err.max():.3e}"


def test_tap_product_premodulated_equals_in_launch(ctx, prec):
    """The tap-product weights modulated ahead (ops.modulate_weights, the engine's side-stream premodulation
    wbs[idx]["conv9"]) against the modulation inside the conv launch: equal products."""
    n, cin, h, w, cout = 2, 64, 9, 7, 32
    _, _, x, s, d, _, cw9 = _layer(n, cin, h, w, cout)
    xs, sv, d9 = NHWC(dev32(x.permute(0, 2, 3, 1))), dev32(s), dev32(d.repeat(1, 9))
    a, b = NHWC.empty(n, h, w, 9 * cout, DEV), NHWC.empty(n, h, w, 9 * cout, DEV)
    ops.modulated_conv2d(ctx, xs, cw9, a, sv, d9)
    ops.modulated_conv2d(ctx, xs, cw9, b, sv, d9, premod=ops.modulate_weights(ctx, cw9, sv, d9, n))
    torch.cuda.synchronize()
    assert torch.isfinite(a.t).all() and a.t.abs().max() > 0.1 and torch.equal(a.t, b.t)


@pytest.fixture(scope="module")
def enet_b2():
    """ENet with synthetic weights and NoiseInjection weight 0.1 on every StyleConv, and a B = 2 input."""
    from s2v_amd import models
    from s2v_amd.models import arch
    sd = synth.synth_torch_state_dict(arch.ENetParams(lnet=arch.LNetParams()), noise_weight=0.1)
    model = models.ENet()
    model.load_state_dict(sd, strict=True)
    mel, face, gt = synth.lipsync_inputs("enet.tapsum", 2, 256)
    return model.eval(), [torch.from_numpy(a).to(DEV) for a in (mel, face, gt)]


def _tail_convs(model, inputs, noises, monkeypatch):
    """One eager forward; returns (out, the conv launches of the forward as (kh, cin, cout, h, w))."""
    seen = []

    def hook(ctx, info, flops, go):
        seen.append((info.kh, info.cin, info.cout, info.h, info.w))
        go()
    monkeypatch.setattr(ops, "CONV_HOOK", hook)
    out = model(*inputs, noises=noises)[0].clone()
    torch.cuda.synchronize()
    monkeypatch.setattr(ops, "CONV_HOOK", None)
    return out, seen


@pytest.mark.parametrize("crop", [True, False])
def test_enet_tapsum_against_polyphase(enet_b2, monkeypatch, crop):
    """The engine at B = 2 with S2V_ENET_TAPSUM=1 against =0 (module flag), cropped and full-frame tail, the same
    caller-passed noise planes: out within test_models_gpu.py's f16x3 ENet bound; the tap-product tail launches no
    d2s conv (3x3 256 -> 4 x 128) and, in the full-frame form, no strip convs (3x3 over 8-line strip images)."""
    model, inputs = enet_b2
    noises = [dev32(rnd(2, r, r, seed=31 + i)) for i, r in enumerate((200, 200, 400, 400))]
    monkeypatch.setattr(E, "CROP_TAIL", crop)
    assert E.TAPSUM
    out1, convs1 = _tail_convs(model, inputs, noises, monkeypatch)
    monkeypatch.setattr(E, "TAPSUM", False)
    out0, convs0 = _tail_convs(model, inputs, noises, monkeypatch)

    tail_in = (196, 196) if crop else (200, 200)      # StyleConv 3's input (the style encoder has no such size)

    def d2s(c):
        return c[0] == 3 and c[1:3] == (256, 4 * 128) and c[3:5] == tail_in

    def strip(c):
        return c[0] == 3 and c[1:3] == (256, 128) and sorted(c[3:5]) == [8, 400]

    def tap(c):
        return c[0] == 1 and c[1:3] == (256, 9 * 128) and c[3:5] == tail_in
    assert sum(map(d2s, convs0)) == 1 and sum(map(strip, convs0)) == (0 if crop else 2) and not any(map(tap, convs0))
    assert sum(map(tap, convs1)) == 1 and not any(map(d2s, convs1)) and not any(map(strip, convs1))
    assert len(convs1) == len(convs0) - (0 if crop else 2)
    err = (out1 - out0).abs()
    print(f"enet tapsum vs polyphase (crop={crop}): max {err.max():.3e} mean {err.mean():.3e}")
    assert torch.isfinite(out1).all() and err.max() <= ENET_TOL_F16X3[0] and err.mean() <= ENET_TOL_F16X3[1]
