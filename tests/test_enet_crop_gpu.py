"""ENet's cropped StyleConv tail (engine/enet.py CROP_TAIL): the tail computed only on the pixels that reach the
[8:-8, 8:-8] output ENet keeps must give those pixels bit for bit the values of the full-frame tail.

Every comparison here is torch.equal: the cropped tail runs the same kernels over the same taps in the same order,
so there is no tolerance to state.  Pieces first (ToRGB with frame origins in both output modes, unpadded modulated
convs against the interior of the padded ones, direct and polyphase), then the whole engine eager and graph-replayed,
then the cone arithmetic on the CPU."""
import math

import pytest
import torch

import s2v_import  # noqa: F401
from s2v_amd import ops, synth
from s2v_amd.engine import enet as E
from s2v_amd.ops import NHWC, ConvW

DEV = "cuda"


@pytest.fixture(scope="module")
def ctx():
    return ops.Ctx(DEV)


def rnd(*shape, seed=0, lo=-1.0, hi=1.0):
    g = torch.Generator().manual_seed(seed)
    return (lo + (hi - lo) * torch.rand(*shape, generator=g, dtype=torch.float64)).float()


def nhwc(t):
    """[N, H, W, C] host tensor -> dense NHWC device view."""
    return NHWC(t.contiguous().to(DEV))


# (output window origin, size, skip window origin, size) in the 12 x 12 frame over a 6 x 6 skip frame: the second
# window has h * w = 63 (no multiple of 32: the kernel's guarded last block) and a skip window that is not the frame
WINDOWS = [((2, 2), (8, 8), (0, 0), (6, 6)), ((1, 3), (9, 7), (0, 1), (6, 5))]


@pytest.mark.gpu
@pytest.mark.parametrize("win", WINDOWS)
def test_torgb_up2_window_equals_full_frame(ctx, win):
    """ops.torgb_up2 on a window of the frame (frame=, origin=, skip_origin=) against the whole-frame call sliced
    to the window, NHWC output; and the NCHW output mode (crop=) against the transposed, cropped NHWC result of the
    same window, with crops (0, 0) and (1, 2)."""
    (oy, ox), (h, w), (sy, sx), (sh, sw) = win
    n, c, fh, fw = 2, 32, 12, 12
    x = rnd(n, fh, fw, c, seed=1)
    skip = rnd(n, fh // 2, fw // 2, 4, seed=2)
    s = rnd(n, c, seed=3, lo=0.5, hi=1.5).to(DEV)
    cw = ConvW(rnd(3, c, 1, 1, seed=4) / math.sqrt(c), rnd(3, seed=5), DEV)
    full = NHWC.empty(n, fh, fw, 4, DEV)
    ops.torgb_up2(ctx, nhwc(x), cw, s, nhwc(skip), full)
    want = full.t[:, oy: oy + h, ox: ox + w].clone()
    xw, kw = nhwc(x[:, oy: oy + h, ox: ox + w]), nhwc(skip[:, sy: sy + sh, sx: sx + sw])
    got = NHWC.empty(n, h, w, 4, DEV)
    ops.torgb_up2(ctx, xw, cw, s, kw, got, frame=(fh, fw), origin=(oy, ox), skip_origin=(sy, sx))
    torch.cuda.synchronize()
    assert torch.equal(got.t, want)
    for cy, cx in ((0, 0), (1, 2)):
        planes = torch.full((n, 3, h - 2 * cy, w - 2 * cx), float("nan"), device=DEV)
        ops.torgb_up2(ctx, xw, cw, s, kw, planes, frame=(fh, fw), origin=(oy, ox), skip_origin=(sy, sx), crop=(cy, cx))
        torch.cuda.synchronize()
        assert torch.equal(planes, want[:, cy: h - cy, cx: w - cx, :3].permute(0, 3, 1, 2).contiguous())


@pytest.mark.gpu
def test_torgb_up2_refuses_a_window_past_the_skip(ctx):
    """An output window whose bilinear taps leave the skip window is an error, not an out-of-bounds read."""
    n, c = 1, 32
    cw = ConvW(rnd(3, c, 1, 1, seed=4), None, DEV)
    s = rnd(n, c, seed=3).to(DEV)
    x, y = nhwc(rnd(n, 8, 8, c, seed=1)), NHWC.empty(n, 8, 8, 4, DEV)
    with pytest.raises(Exception, match="outside the 4x4 skip window"):      # rows 2..9 read skip rows 0..5
        ops.torgb_up2(ctx, x, cw, s, nhwc(rnd(n, 4, 4, 4, seed=2)), y, frame=(12, 12), origin=(2, 2), skip_origin=(1, 1))
    with pytest.raises(Exception, match="leaves the 12x12 frame"):
        ops.torgb_up2(ctx, x, cw, s, nhwc(rnd(n, 6, 6, 4, seed=2)), y, frame=(12, 12), origin=(5, 2))


def _tile(prec):
    """force_tile of the 64 x 64 tile in the precision's table (conv_plan.cpp kTiles / kX3Tiles)."""
    return 4 if prec == "f32" else 5


@pytest.mark.gpu
def test_unpadded_modconv_equals_padded_interior(ctx, prec):
    """Modulated, demodulated 3x3 32 -> 32 with noise on 2 x 12 x 12: padding=(0, 0) on the conv's own packed
    weights against rows / columns 1..10 of the padded conv, same tile."""
    n, c, h = 2, 32, 12
    cw = ConvW(rnd(c, c, 3, 3, seed=11) / math.sqrt(9 * c), rnd(c, seed=12), DEV, padding=1)
    x = nhwc(rnd(n, h, h, c, seed=13))
    s = rnd(n, c, seed=14, lo=0.5, hi=1.5).to(DEV)
    d = rnd(n, c, seed=15, lo=0.5, hi=1.5).to(DEV)
    noise = rnd(n, h, h, seed=16).to(DEV)
    kw = dict(act=ops.ACT_LRELU, alpha=0.2, pix_w=0.1, force_tile=_tile(prec))
    full = NHWC.empty(n, h, h, c, DEV)
    ops.modulated_conv2d(ctx, x, cw, full, s, d, pix_add=noise, **kw)
    got = NHWC.empty(n, h - 2, h - 2, c, DEV)
    ops.modulated_conv2d(ctx, x, cw, got, s, d, pix_add=noise[:, 1:-1, 1:-1].contiguous(), padding=(0, 0), **kw)
    torch.cuda.synchronize()
    assert torch.equal(got.t, full.t[:, 1:-1, 1:-1])


@pytest.mark.gpu
def test_unpadded_polyphase_modconv_equals_padded_interior(ctx, prec):
    """The depth-to-space polyphase form (x2 upsample folded into four parity-class filters) 32 -> 4 x 32 on
    2 x 10 x 10: padding=(0, 0) gives input pixels 1..8, i.e. output rows / columns 2..17 of the 20 x 20 padded
    result, with the noise plane's window."""
    n, c, h = 2, 32, 10
    w = rnd(c, c, 3, 3, seed=21) / math.sqrt(9 * c)
    cw4 = ConvW(E.fold_up2_conv3(w), rnd(c, seed=22).repeat(4), DEV, padding=1)
    x = nhwc(rnd(n, h, h, c, seed=23))
    s = rnd(n, c, seed=24, lo=0.5, hi=1.5).to(DEV)
    d4 = rnd(n, c, seed=25, lo=0.5, hi=1.5).repeat(1, 4).contiguous().to(DEV)
    noise = rnd(n, 2 * h, 2 * h, seed=26).to(DEV)
    kw = dict(act=ops.ACT_LRELU, alpha=0.2, pix_w=0.1, d2s=True, force_tile=_tile(prec))
    full = NHWC.empty(n, 2 * h, 2 * h, c, DEV)
    ops.modulated_conv2d(ctx, x, cw4, full, s, d4, pix_add=noise, **kw)
    got = NHWC.empty(n, 2 * h - 4, 2 * h - 4, c, DEV)
    ops.modulated_conv2d(ctx, x, cw4, got, s, d4, pix_add=noise[:, 2:-2, 2:-2].contiguous(), padding=(0, 0), **kw)
    torch.cuda.synchronize()
    assert torch.equal(got.t, full.t[:, 2:-2, 2:-2])


@pytest.fixture(scope="module")
def enet_b2():
    """ENet with synthetic weights and NoiseInjection weight 0.1 on every StyleConv, and a B = 2 input."""
    from s2v_amd import models
    from s2v_amd.models import arch
    sd = synth.synth_torch_state_dict(arch.ENetParams(lnet=arch.LNetParams()), noise_weight=0.1)
    model = models.ENet()
    model.load_state_dict(sd, strict=True)
    mel, face, gt = synth.lipsync_inputs("enet.crop", 2, 256)
    return model.eval(), [torch.from_numpy(a).to(DEV) for a in (mel, face, gt)]


def _planes(n):
    return [rnd(n, r, r, seed=31 + i).to(DEV) for i, r in enumerate((200, 200, 400, 400))]


@pytest.mark.gpu
def test_enet_cropped_tail_equals_full_tail(enet_b2, monkeypatch):
    """out / low of the whole engine with the cropped tail against the full-frame tail (S2V_ENET_CROP_TAIL=0's
    path, selected through the module flag) in one process: with caller-passed noise planes, and with planes
    drawn by the forward (the full-tail run is then fed the planes the cropped run drew, read from last_noises,
    which keep their full [B, 200 | 400, 200 | 400] shapes)."""
    model, inputs = enet_b2
    eng = model._engine(inputs[0].device)[0]
    assert E.CROP_TAIL and eng._crop_cone(100, torch.empty(2, 3, 384, 384, device="meta")) is not None
    noises = _planes(2)
    out1, low1 = (t.clone() for t in model(*inputs, noises=noises))
    assert eng.last_noises == [None] * 4
    out2, low2 = (t.clone() for t in model(*inputs))                    # planes drawn on the device
    drawn = [p.clone() for p in eng.last_noises]
    assert [tuple(p.shape) for p in drawn] == [(2, 200, 200), (2, 200, 200), (2, 400, 400), (2, 400, 400)]
    monkeypatch.setattr(E, "CROP_TAIL", False)
    assert eng._crop_cone(100, out1) is None
    ref1, rlow1 = (t.clone() for t in model(*inputs, noises=noises))
    ref2, rlow2 = (t.clone() for t in model(*inputs, noises=drawn))
    torch.cuda.synchronize()
    assert torch.isfinite(out1).all() and (out1 - out2).abs().max() > 1e-3       # the noise reaches the output
    assert torch.equal(out1, ref1) and torch.equal(low1, rlow1)
    assert torch.equal(out2, ref2) and torch.equal(low2, rlow2)


@pytest.mark.gpu
def test_enet_cropped_tail_graph_replay_equals_eager(enet_b2, monkeypatch):
    """The cropped tail captured as bench.py captures the step (runtime.GraphRunner) and replayed: the replay
    equals the eager full-frame tail fed the planes that replay drew."""
    from s2v_amd.runtime import GraphRunner
    model, inputs = enet_b2
    eng = model._engine(inputs[0].device)[0]
    runner = GraphRunner(lambda m, f, g: model(m, f, g), inputs, warmup=1)
    runner.replay()
    out, low = (t.clone() for t in runner.replay())
    drawn = [p.clone() for p in eng.last_noises]
    assert [tuple(p.shape) for p in drawn] == [(2, 200, 200), (2, 200, 200), (2, 400, 400), (2, 400, 400)]
    monkeypatch.setattr(E, "CROP_TAIL", False)
    ref, rlow = model(*inputs, noises=drawn)
    torch.cuda.synchronize()
    assert torch.equal(out, ref) and torch.equal(low, rlow)


def test_crop_tail_cone_arithmetic():
    """The dependency cone and the computed windows for ENet's 100^2 tail input and crop 8 (frame rows, inclusive
    for ``need``; (origin, size) for ``win``), and the crops the unpadded chain cannot serve."""
    cone = E.crop_tail_cone(100, 8)
    assert cone["need"] == {"rgb1": (8, 391), "conv4": (8, 391), "conv3": (7, 392), "rgb0": (3, 196),
                            "conv2": (2, 197), "conv1": (1, 198)}
    assert cone["win"] == {"conv1": (1, 198), "conv2": (2, 196), "rgb0": (2, 196), "conv3": (6, 388),
                           "conv4": (7, 386), "rgb1": (7, 386)}
    assert (cone["crop"], cone["out"]) == (1, 384)
    # the polyphase StyleConv reads input pixels 3..196 for output rows 7..392
    assert (cone["need"]["conv3"][0] // 2, cone["need"]["conv3"][1] // 2) == (3, 196)
    for crop in (0, 1, 2):                      # the cone touches the lines the polyphase fold gets wrong
        assert E.crop_tail_cone(100, crop) is None
    for crop in (3, 4, 5, 6):                   # clear of those lines, but outside the unpadded chain's windows
        assert E.crop_tail_cone(100, crop) is None
    assert E.crop_tail_cone(100, 7)["crop"] == 0 and E.crop_tail_cone(100, 7)["out"] == 386
    assert E.crop_tail_cone(100, 9)["crop"] == 2
    assert E.crop_tail_cone(100, 200) is None   # nothing left
