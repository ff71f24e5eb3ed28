"""The quad epilogue of the implicit-GEMM tiles (conv_impl.hpp epilogue_tile_map) against fp64 CPU
references, on every tile family that shares it: the per-pixel operand (pix_add) staged in the padding
floats of the C rows, the load-free row loops of the common launches and the loops with loads that
the residual / per-(image, channel) scale / SFT / second-output launches keep.

Shapes are the smallest at which a row can go wrong: 3 images of 10 x 10 outputs (M = 300: a ragged
last 64-row chunk and a ragged last tile, rows of one chunk in two images), depth-to-space output with
ow = 10 (the column wrap several times inside a chunk, the noise index the upsampled pixel), per-sample
weights (batch index > 0) and cout = 136 / 4 x 40 (dead quads in the last N tile).  pix_add is the pixel
index scaled by 2^-5, so a value taken from another row is off by >= 0.03, far outside the bounds.

Bounds: those of tests/test_ops_gpu.py for each arithmetic (REL * sum|a*b| forms), with the magnitude
of the added per-pixel term inside the sum."""
import functools
import math

import pytest
import torch
import torch.nn.functional as F

import s2v_import  # noqa: F401

pytestmark = pytest.mark.gpu

from s2v_amd import ops  # noqa: E402
from s2v_amd.ops import NHWC, ConvW  # noqa: E402

DEV = "cuda"
REL = {"f32": 2e-6, "bf16x3": 5e-5, "f16x3": 3e-6}

# (precision, force_tile): the split-precision tiles 256x256 (1), 128x128 (2), 64x64 (5), 512x128 (9) and
# 256x64 with 4 waves (11); the fp32 table's 128x128 (1) and 64x64 (4)
X3 = [(p, t) for p in ("f16x3", "bf16x3") for t in (1, 2, 5, 9, 11)]
COMBOS = X3 + [("f32", 1), ("f32", 4)]
IDS = [f"{p}-t{t}" for p, t in COMBOS]
N, CIN, H, W, COUT = 3, 32, 10, 10, 136
PIX_W = 1.0


@pytest.fixture(scope="module")
def ctx():
    return ops.Ctx(DEV)


@pytest.fixture(params=COMBOS, ids=IDS)
def mode(request):
    prev = ops.set_precision(request.param[0])
    yield request.param
    ops.set_precision(prev)


def nhwc(t):
    return NHWC(t.permute(0, 2, 3, 1).contiguous().to(DEV))


def to_nchw(v):
    return v.t[..., v.coff: v.coff + v.c].permute(0, 3, 1, 2).double().cpu()


def rnd(*shape, seed=0, lo=-1.0, hi=1.0):
    g = torch.Generator().manual_seed(seed)
    return lo + (hi - lo) * torch.rand(*shape, generator=g, dtype=torch.float64)


def pixel_index(n, h, w):
    """One distinct value per output pixel (exact in fp32)."""
    return torch.arange(n * h * w, dtype=torch.float64).reshape(n, h, w) / 32.0


@functools.lru_cache(maxsize=None)
def dense():
    """Inputs and fp64 results shared by the dense-output cases."""
    wt = rnd(COUT, CIN, 3, 3, seed=1) / math.sqrt(CIN * 9)
    bias = rnd(COUT, seed=2)
    x = rnd(N, CIN, H, W, seed=3)
    conv = F.conv2d(x, wt, bias, padding=1)
    bound = F.conv2d(x.abs(), wt.abs(), padding=1)
    return dict(wt=wt, bias=bias, x=x, conv=conv, bound=bound, noise=pixel_index(N, H, W),
                res=rnd(N, COUT, H, W, seed=4), ncs=rnd(N, COUT, seed=5, lo=0.5, hi=1.5))


def run_dense(ctx, tile, **kw):
    d = dense()
    cw = ConvW(d["wt"].float(), d["bias"].float(), DEV, padding=1)
    y = NHWC.empty(N, H, W, COUT + 8, DEV).slice(4, COUT)       # a channel slice of a wider tensor
    ops.conv2d(ctx, nhwc(d["x"].float()), cw, y, force_tile=tile, **kw)
    return to_nchw(y)


def check(got, ref, lim, what):
    err = (got - ref).abs()
    print(f"{what}: max err {err.max():.3e}, worst err / bound {(err / lim).max():.3f}")
    assert (err <= lim).all(), f"{what}: max err {err.max():.3e}, err / bound {(err / lim).max():.2f}"


def test_pix_add_dense(ctx, mode):
    """Noise on a dense output, LeakyReLU: the load-free row loop, noise from pad 0 of each row."""
    prec, tile = mode
    d = dense()
    got = run_dense(ctx, tile, act=ops.ACT_LRELU, alpha=0.2, pix_add=d["noise"].float().to(DEV), pix_w=PIX_W)
    ref = F.leaky_relu(d["conv"] + PIX_W * d["noise"][:, None], 0.2)
    lim = REL[prec] * (d["bound"] + (PIX_W * d["noise"][:, None]).abs() + 1) + 1e-6
    check(got, ref, lim, "pix_add dense")


@pytest.mark.parametrize("after", [False, True])
def test_residual_quads(ctx, mode, after):
    """Residual before / after the activation: the row loop that keeps its loads."""
    prec, tile = mode
    d = dense()
    got = run_dense(ctx, tile, act=ops.ACT_LRELU, alpha=0.2, res=nhwc(d["res"].float()), res_after=after)
    ref = F.leaky_relu(d["conv"], 0.2) + d["res"] if after else F.leaky_relu(d["conv"] + d["res"], 0.2)
    check(got, ref, REL[prec] * (d["bound"] + 1) + 1e-6, f"res_after={after}")


def test_nc_scale_with_pix_add(ctx, mode):
    """Per-(image, channel) scale + noise + tanh: the generic loop (out-of-line activation), noise from the pad."""
    prec, tile = mode
    d = dense()
    b = d["bias"][None, :, None, None]
    got = run_dense(ctx, tile, act=ops.ACT_TANH, nc_scale=d["ncs"].float().to(DEV),
                    pix_add=d["noise"].float().to(DEV), pix_w=0.125)
    ref = torch.tanh((d["conv"] - b) * d["ncs"][:, :, None, None] + b + 0.125 * d["noise"][:, None])
    lim = 1.5 * (REL[prec] * (d["bound"] + (0.125 * d["noise"][:, None]).abs() + 1) + 1e-6)
    check(got, ref, lim, "nc_scale + pix_add")


def test_post_and_dup(ctx, mode):
    """SFT on the upper channels and the second output (bounds of test_conv2d_post_and_dup_epilogue)."""
    prec, tile = mode
    d = dense()
    c0 = 64
    pm, pa = rnd(N, COUT - c0, H, W, seed=75), rnd(N, COUT - c0, H, W, seed=76)
    ds, db = rnd(N, COUT, H, W, seed=77), rnd(COUT, seed=78)
    cw = ConvW(d["wt"].float(), d["bias"].float(), DEV, padding=1)
    full = NHWC.empty(N, H, W, 2 * COUT, DEV)
    ops.conv2d(ctx, nhwc(d["x"].float()), cw, full.slice(0, COUT), act=ops.ACT_LRELU, alpha=0.2, force_tile=tile,
               post=(nhwc(pm.float()), nhwc(pa.float()), c0), dup=(nhwc(ds.float()), db.float().to(DEV), 0.7, COUT))
    v = F.leaky_relu(d["conv"], 0.2)
    bound = d["bound"].clone()
    v[:, c0:] = v[:, c0:] * pm + pa
    bound[:, c0:] = bound[:, c0:] * pm.abs()
    got = to_nchw(full)
    check(got[:, :COUT], v, REL[prec] * (bound + 1) + 1e-6, "post")
    dref = F.leaky_relu(0.7 * ds + db[None, :, None, None], 0.2)
    assert (got[:, COUT:] - dref).abs().max() < 1e-6


@functools.lru_cache(maxsize=None)
def modulated(d2s):
    cout = 40 if d2s else COUT
    wt = rnd(cout, CIN, 3, 3, seed=31) / math.sqrt(CIN * 9)
    bias = rnd(cout, seed=32)
    x = rnd(N, CIN, H, W, seed=33)
    s = rnd(N, CIN, seed=34, lo=0.5, hi=1.5)
    dm = rnd(N, cout, seed=35, lo=0.5, hi=1.5)
    wb = wt[None] * s[:, None, :, None, None] * dm[:, :, None, None, None]
    src = F.interpolate(x, scale_factor=2, mode="bilinear", align_corners=False) if d2s else x
    f = 2 if d2s else 1
    noise = pixel_index(N, f * H, f * W)
    conv = torch.stack([F.conv2d(src[i:i + 1], wb[i], bias, padding=1)[0] for i in range(N)])
    bound = torch.stack([F.conv2d(src[i:i + 1].abs(), wb[i].abs(), padding=1)[0] for i in range(N)])
    ref = F.leaky_relu(conv + PIX_W * noise[:, None], 0.2)
    return dict(wt=wt, bias=bias, x=x, s=s, dm=dm, noise=noise, ref=ref,
                bound=bound + (PIX_W * noise[:, None]).abs() + 1)


def force_modulated_tile(monkeypatch, x, cw, y, tile, d2s):
    """modulated_conv2d takes its forced tile from the perf table: one entry for this launch."""
    if ops.PRECISION == "f32" or not tile:
        return                     # (the fp32 arithmetic does not read the table: the planner's own tile)
    key = ops.conv_key(x, cw, y.v, 1, False, ops.prec_code()) + f"|mod1{int(d2s)}"
    monkeypatch.setattr(ops, "PERFDB", {key: (tile, 0)})
    monkeypatch.setitem(ops._PERFDB_MATCH, str(x.t.device), True)


def test_batch_pix_add(ctx, mode, monkeypatch):
    """Per-sample weights (batch index > 0), noise per sample, M = 100 per sample (ragged chunk and tile)."""
    prec, tile = mode
    d = modulated(False)
    cw = ConvW(d["wt"].float(), d["bias"].float(), DEV, padding=1)
    x = nhwc(d["x"].float())
    y = NHWC.empty(N, H, W, COUT + 4, DEV).slice(0, COUT)
    force_modulated_tile(monkeypatch, x, cw, y, tile, False)
    ops.modulated_conv2d(ctx, x, cw, y, d["s"].float().to(DEV), d["dm"].float().to(DEV), act=ops.ACT_LRELU, alpha=0.2,
                         pix_add=d["noise"].float().to(DEV).contiguous(), pix_w=PIX_W)
    check(to_nchw(y), d["ref"], 2 * REL[prec] * d["bound"] + 1e-6, "batch pix_add")


def test_d2s_pix_add(ctx, mode, monkeypatch):
    """Depth-to-space output, ow = 10, noise indexed by the upsampled pixel (2 oy + dy, 2 ox + dx); as
    test_modulated_conv_d2s_polyphase, away from the two outermost output lines of each side."""
    from s2v_amd.engine.enet import fold_up2_conv3
    prec, tile = mode
    d = modulated(True)
    cw4 = ConvW(fold_up2_conv3(d["wt"].float()), d["bias"].float().repeat(4), DEV, padding=1)
    x = nhwc(d["x"].float())
    y = NHWC.empty(N, 2 * H, 2 * W, 40, DEV)
    force_modulated_tile(monkeypatch, x, cw4, y, tile, True)
    ops.modulated_conv2d(ctx, x, cw4, y, d["s"].float().to(DEV), d["dm"].float().repeat(1, 4).to(DEV),
                         act=ops.ACT_LRELU, alpha=0.2, pix_add=d["noise"].float().to(DEV), pix_w=PIX_W, d2s=True)
    inner = (slice(None), slice(None), slice(2, -2), slice(2, -2))
    check(to_nchw(y)[inner], d["ref"][inner], 4 * REL[prec] * d["bound"][inner] + 1e-6, "d2s pix_add")
