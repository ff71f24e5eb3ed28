"""Shared cases of the single-pass f16 conv arithmetic ("f16") tests and measurements: the smallest shapes
at which the ELT 2 kernels can go wrong (taken from tests/test_ops_gpu.py CONV_CASES and its halo / grid_cap /
group tests), their fp64 references, a launcher, and the CPU emulation of the mode on the reference math
(every F.conv2d / F.conv_transpose2d operand of oracle.nets rounded to 11 significant bits)."""
import contextlib
import math

import torch
import torch.nn.functional as F

DEV = "cuda"
REL_F32 = 2e-6          # tests/test_ops_gpu.py REL["f32"], by value: the fp32 sums of an MFMA conv
REL_F16 = 1e-3          # per product (1 + 2^-11)^2 - 1 = 9.77e-4, plus the 2e-6 of the sums


def rnd(*shape, seed=0, lo=-1.0, hi=1.0):
    g = torch.Generator().manual_seed(seed)
    return lo + (hi - lo) * torch.rand(*shape, generator=g, dtype=torch.float64)


class Case:
    """One launch: a conv (``tile`` / ``splits``: force_tile / force_splits, ``cap``: ops.x3_grid_cap blocks), or a
    conv group (``group``: members (c0, c1, cout), 3x3 valid convs over channels [c0, c1) of one input)."""

    def __init__(self, name, n, cin, h, w, cout, k=3, stride=1, pad=1, mode="direct", pad_mode="zero", tile=0,
                 splits=0, cap=0, group=None):
        self.name, self.n, self.cin, self.h, self.w, self.cout, self.k = name, n, cin, h, w, cout, k
        self.stride, self.pad, self.mode, self.pad_mode = stride, pad, mode, pad_mode
        self.tile, self.splits, self.cap, self.group = tile, splits, cap, group

    def members(self):
        return self.group if self.group else [(0, self.cin, self.cout)]

    def __repr__(self):
        return self.name


CASES = [
    Case("planner", 2, 64, 17, 19, 96),                                        # ragged M and N, planner's tile
    Case("tile1_256x256", 2, 64, 16, 16, 256, tile=1),
    Case("tile2_3splits", 2, 64, 16, 16, 128, tile=2, splits=3),
    Case("tile3_stride2", 1, 32, 20, 12, 64, stride=2, tile=3),
    Case("tile5_cout_lt_bn", 2, 32, 12, 12, 32, tile=5),
    Case("tile5_reflect_2splits", 2, 64, 17, 15, 32, pad_mode="reflect", tile=5, splits=2),
    Case("up2_prologue", 2, 32, 8, 8, 48, mode="up2"),
    Case("halo_4x64", 2, 64, 8, 64, 64, tile=18),
    Case("halo_8x64", 2, 64, 8, 64, 64, tile=19),
    Case("halo_4x64x128", 2, 64, 8, 64, 64, tile=20),
    Case("persist_cap8", 2, 64, 64, 64, 160, tile=1, cap=8),
    Case("group2", 2, 256, 14, 14, 0, pad=0, group=[(0, 256, 64), (0, 64, 192)]),
]


def weights(case, exact, seed=1):
    """Per member (wt [cout, c, k, k], bias [cout]) in fp64.  ``exact``: w = m / 16 with m in [-8, 8] and bias = j / 128,
    else the project's rnd weights as test_conv2d builds them."""
    out = []
    for i, (c0, c1, cout) in enumerate(case.members()):
        c = c1 - c0
        if exact:
            g = torch.Generator().manual_seed(seed + 10 * i)
            wt = torch.randint(-8, 9, (cout, c, case.k, case.k), generator=g).double() / 16
            b = torch.randint(-128, 129, (cout,), generator=g).double() / 128
        else:
            wt = rnd(cout, c, case.k, case.k, seed=seed + 10 * i) / math.sqrt(c * case.k * case.k)
            b = rnd(cout, seed=seed + 10 * i + 1)
        out.append((wt, b))
    return out


def inputs(case, exact, seed=3):
    if exact:                                         # x = k / 8 with integer k in [-64, 64]
        g = torch.Generator().manual_seed(seed)
        return torch.randint(-64, 65, (case.n, case.cin, case.h, case.w), generator=g).double() / 8
    return rnd(case.n, case.cin, case.h, case.w, seed=seed)


def _prep(case, x):
    xin = F.interpolate(x, scale_factor=2, mode="nearest") if case.mode == "up2" else x
    if case.pad_mode == "reflect":
        return F.pad(xin, (case.pad,) * 4, mode="reflect"), 0
    return xin, case.pad


def reference(case, x, ws, xmap=lambda t: t, wmap=lambda t, i: t):
    """Per member (conv64(xmap(x), wmap(w)) + bias, sum |x| |w|): the fp64 reference and the error bound's scale."""
    out = []
    for i, ((c0, c1, _), (wt, b)) in enumerate(zip(case.members(), ws)):
        xp, p = _prep(case, x[:, c0:c1])
        ref = F.conv2d(xmap(xp), wmap(wt, i), b, case.stride, p)
        bound = F.conv2d(xp.abs(), wt.abs(), None, case.stride, p)
        out.append((ref, bound))
    return out


def conv_weights(case, ws):
    from s2v_amd import ops
    return [ops.ConvW(wt.float(), b.float(), DEV, stride=case.stride, padding=case.pad,
                      pad_mode=ops.PAD_REFLECT if case.pad_mode == "reflect" else ops.PAD_ZERO,
                      in_mode=ops.IN_NEAREST_UP2 if case.mode == "up2" else ops.IN_DIRECT) for wt, b in ws]


def launch(ctx, case, x, cws, epi=lambda i, shape: {}, wide=False):
    """Run the case on the device in the current precision -> per member the NCHW fp64 output.  ``epi(i, shape)``:
    extra conv2d arguments of member i (shape = its NCHW output shape); ``wide``: the output is a channel
    slice of a wider tensor."""
    from s2v_amd import ops
    from s2v_amd.ops import NHWC
    xv = NHWC(x.float().permute(0, 2, 3, 1).contiguous().to(DEV))
    up = 2 if case.mode == "up2" else 1
    oh = (up * case.h + 2 * case.pad - case.k) // case.stride + 1
    ow = (up * case.w + 2 * case.pad - case.k) // case.stride + 1
    ys = []
    with ops.x3_grid_cap(ctx, case.cap) if case.cap else contextlib.nullcontext():
        with ops.conv_group(ctx) if case.group else contextlib.nullcontext():
            for i, (c0, c1, cout) in enumerate(case.members()):
                y = NHWC.empty(case.n, oh, ow, cout + 5, DEV).slice(3, cout) if wide else NHWC.empty(case.n, oh, ow,
                                                                                                  cout, DEV)
                xs = xv.slice(c0, c1 - c0) if case.group else xv
                ops.conv2d(ctx, xs, cws[i], y, force_tile=case.tile, force_splits=case.splits,
                           **epi(i, (case.n, cout, oh, ow)))
                ys.append(y)
    torch.cuda.synchronize()
    return [y.t[..., y.coff: y.coff + y.c].permute(0, 3, 1, 2).double().cpu() for y in ys]


# ----------------------------------------------------------------------------- CPU emulation of the mode
def round_operand(t, top, bits=11):
    """``t`` rounded to ``bits`` significant bits (11: f16, 8: bf16) after the power-of-two scale that puts max |t|
    into [2^top, 2^(top + 1)) — the way the weight packer (top 13) and the range guard (top 9) scale operands."""
    m = float(t.abs().max())
    if not (m > 0) or not math.isfinite(m):
        return t
    s = 2.0 ** (top - math.floor(math.log2(m)))
    r = (t.float() * s).half() if bits == 11 else (t.float() * s).bfloat16()
    return (r.to(t.dtype)) / s


@contextlib.contextmanager
def emulate(bits=11):
    """While active, torch.nn.functional.conv2d / conv_transpose2d round both operands (round_operand) before the
    reference's own fp32 convolution: what the oracle computes under single-pass 16-bit products."""
    c2, ct = F.conv2d, F.conv_transpose2d

    def conv2d(x, w, *a, **k):
        return c2(round_operand(x, 9, bits), round_operand(w, 13, bits), *a, **k)

    def conv_transpose2d(x, w, *a, **k):
        return ct(round_operand(x, 9, bits), round_operand(w, 13, bits), *a, **k)
    F.conv2d, F.conv_transpose2d = conv2d, conv_transpose2d
    try:
        yield
    finally:
        F.conv2d, F.conv_transpose2d = c2, ct


def oracle_outputs(model):
    """The CPU oracle's outputs on the golden inputs of ``model`` ('lnet', 'enet', 'dnet', 'gfpgan'), keyed as
    profiles/f16_precision.json keys them."""
    from helpers import synth_sd
    from s2v_amd import synth
    sd = synth_sd(model)
    with torch.no_grad():
        if model == "lnet":
            from oracle import nets
            mel, face, _ = synth.lipsync_inputs("golden.lnet", 2, 96)
            return {"lnet_out": nets.lnet_forward(sd, torch.from_numpy(mel), torch.from_numpy(face))}
        if model == "enet":
            from oracle import nets
            mel, face, gt = synth.lipsync_inputs("golden.enet256", 1, 256)
            o, low = nets.enet_forward(sd, torch.from_numpy(mel), torch.from_numpy(face), torch.from_numpy(gt))
            return {"enet_out": o, "enet_out_clamped": o.clamp(0, 1), "enet_low": low}
        if model == "dnet":
            from oracle import nets
            src, coeff = synth.dnet_inputs("golden.dnet128", 2, 128)
            o = nets.dnet_forward(sd, torch.from_numpy(src), torch.from_numpy(coeff))
            return {"dnet_flow": o["flow_field"], "dnet_warp_image": o["warp_image"], "dnet_fake_image": o["fake_image"]}
        from oracle import enhancers
        x = torch.from_numpy(synth.face_inputs("golden.gfpgan", 1))
        img, rgbs, _ = enhancers.gfpgan_forward(sd, x, return_rgb=True)
        return {"gfpgan_out": img, "gfpgan_rgb0": rgbs[0], "gfpgan_rgb3": rgbs[3]}


def emulation_figures(model, bits=11):
    """{output: (max, mean) |emulated - plain|} of the oracle of ``model``."""
    plain = oracle_outputs(model)
    with emulate(bits):
        emu = oracle_outputs(model)
    return {k: (float((emu[k] - plain[k]).abs().max()), float((emu[k] - plain[k]).abs().mean())) for k in plain}


# ----------------------------------------------------------------------------- the models on the device
def build_model(model):
    from helpers import GFPGAN_KW, synth_sd
    from s2v_amd import models
    m = {"lnet": models.LNet, "enet": models.ENet, "dnet": models.DNet,
         "gfpgan": lambda: models.GFPGANv1Clean(**GFPGAN_KW)}[model]()
    m.load_state_dict(synth_sd(model), strict=True)
    return m.eval()


def device_outputs(model, net):
    """The device model's outputs on the golden inputs, in the current precision, keyed as oracle_outputs."""
    from s2v_amd import synth

    def dev(a):
        return torch.from_numpy(a).to(DEV)
    if model == "lnet":
        mel, face, _ = synth.lipsync_inputs("golden.lnet", 2, 96)
        return {"lnet_out": net(dev(mel), dev(face))}
    if model == "enet":
        mel, face, gt = synth.lipsync_inputs("golden.enet256", 1, 256)
        o, low = net(dev(mel), dev(face), dev(gt))
        return {"enet_out": o, "enet_out_clamped": o.clamp(0, 1), "enet_low": low}
    if model == "dnet":
        src, coeff = synth.dnet_inputs("golden.dnet128", 2, 128)
        o = net(dev(src), dev(coeff))
        return {"dnet_flow": o["flow_field"], "dnet_warp_image": o["warp_image"], "dnet_fake_image": o["fake_image"]}
    img, rgbs = net(dev(synth.face_inputs("golden.gfpgan", 1)), return_rgb=True, randomize_noise=False)
    return {"gfpgan_out": img, "gfpgan_rgb0": rgbs[0], "gfpgan_rgb3": rgbs[3]}


GOLDEN_OF = {"lnet": "lnet_b2_96", "enet": "enet_b1_256", "dnet": "dnet_b2_128", "gfpgan": "gfpgan_b1_512"}
GOLDEN_KEY = {"lnet_out": "out", "enet_out": "out", "enet_out_clamped": "out", "enet_low": "low", "dnet_flow": "flow",
              "dnet_warp_image": "warp_image", "dnet_fake_image": "fake_image", "gfpgan_out": "out",
              "gfpgan_rgb0": "rgb0", "gfpgan_rgb3": "rgb3"}


def golden_error(key, got, g):
    """(max, mean) |got - golden| of output ``key`` against the reference's golden file ``g`` (a whole tensor, or the
    stored probe points of the large ones)."""
    import numpy as np
    name = GOLDEN_KEY[key]
    got = got.detach().double().cpu().numpy()
    if name in g.files:
        ref = g[name].astype(np.float64)
        if key.endswith("_clamped"):
            ref = ref.clip(0, 1)
        d = np.abs(got - ref)
    else:
        d = np.abs(got.reshape(-1)[g[f"{name}_idx"]] - g[f"{name}_val"].astype(np.float64))
    return float(d.max()), float(d.mean())
