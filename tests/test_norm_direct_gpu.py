"""Direct fp64 parity of the normalisation kernels of csrc/norm.hip (LayerNorm2d, InstanceNorm / ADAIN with its
reflect-padded second output) and the data-movement kernels of csrc/misc.hip (resize, pad_reflect, row_pack),
called through ``ops.*`` at the shapes, views and value ranges where they can go wrong.  tests/norm_cases.py
builds the inputs, references and bounds on the CPU; tests/test_norm_cases_host.py checks there that the cases
reach the paths they are listed for and that the bounds tell a wrong kernel from a right one.

The norms are compared element by element against a rounding bound taken from the reference's own fp64 mean
and rstd (norm_cases' docstring), bilinear resize against ``max(4 * e_ref, 16 * 2^-24 * max|ref64|)``; nearest
resize, pad_reflect, row_pack and the padded InstanceNorm output are bit-exact.  Every output buffer and every
channel beside a sliced input or output is pre-filled with NaN: what a kernel must write has to come out
finite, what it must not touch has to stay NaN, and what it must not read would show in the result.  Run with
``-s`` for the achieved error of every case.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import s2v_import  # noqa: F401

pytestmark = pytest.mark.gpu

import norm_cases as nc  # noqa: E402
from s2v_amd import ops  # noqa: E402
from s2v_amd.ops import NHWC  # noqa: E402

DEV = "cuda"
NAN = float("nan")


@pytest.fixture(scope="module")
def ctx():
    return ops.Ctx(DEV)


def nan_view(n, h, w, c, view) -> NHWC:
    """A NaN-filled [n, h, w, pitch] device tensor and its channel slice [off, off + c)."""
    pitch, off = view
    return NHWC(torch.full((n, h, w, pitch), NAN, device=DEV), off, c)


def put(values: torch.Tensor, view) -> NHWC:
    """``values`` [n, h, w, c] as the channel slice of a new device tensor whose other channels hold NaN."""
    v = nan_view(*values.shape, view)
    v.v.copy_(values.to(DEV))
    return v


def check_canary(v: NHWC, what):
    """The channels of v's tensor outside the view are still NaN, the view itself is finite."""
    t = v.t.cpu()
    inside = torch.zeros(v.cs, dtype=torch.bool)
    inside[v.coff:v.coff + v.c] = True
    assert torch.isnan(t[..., ~inside]).all(), f"{what}: wrote outside its channel slice"
    left = int(torch.isnan(t[..., inside]).sum())
    assert left == 0, f"{what}: {left} output values are NaN (never written, or computed from a canary)"
    assert torch.isfinite(t[..., inside]).all(), f"{what}: non-finite output"


def unchanged(v: NHWC, values, what):
    assert torch.equal(v.v.cpu(), values), f"{what}: the input changed"


def check_bound(got: torch.Tensor, d, what):
    """Every element within its own bound; on failure the worst element and its ratio."""
    bound = nc.bound_of(d)
    err = (got.double() - d["ref64"]).abs()
    ratio = err / bound
    worst = int(torch.argmax(torch.nan_to_num(ratio, nan=float("inf"))))
    at = tuple(int(k) for k in np.unravel_index(worst, tuple(ratio.shape)))
    r = float(ratio.flatten()[worst])
    cpu = max(float(((d[k].double() - d["ref64"]).abs() / bound).max()) for k in ("torch32", "fma32"))
    print(f"{what}: max err={float(err.max()):.2e} worst err / bound={r:.3f} at {at} (CPU float32 {cpu:.3f})")
    assert r <= 1.0, (f"{what}: element {at}: got {float(got[at])!r}, reference {float(d['ref64'][at])!r}, "
                      f"err / bound = {r:.3f}")


# ----------------------------------------------------------------------------- LayerNorm2d
@pytest.mark.parametrize("i,pool", nc.LN_RUNS, ids=nc.LN_IDS)
def test_layernorm2d_fp64(ctx, i, pool):
    """s2v_layernorm2d against layer_norm over (C, H, W) in float64 -> act -> 2x2 mean -> + res: the dense
    four-loads-in-flight, the strided float4 and the scalar statistics; ln_apply4 with its 64-block cap (the
    LN_EPT loop taken twice, with and without a ragged last step), ln_apply4_pool on odd sizes, the scalar
    apply by channel count and by misalignment; statistics blocks without a pixel; a mean 100 times the
    spread; a constant image (variance exactly 0: the output is act(bias) + res bit for bit).

    Measured on MI355X: the worst err / bound over the 19 runs is 0.180 (cap64 pooled, 2.9e-07 absolute; the
    CPU float32 evaluations reach 0.21 there), offset 0.017, const 0.001."""
    d = nc.ln_case(i, pool)
    s = d["spec"]
    n, h, w, c = s["n"], s["h"], s["w"], s["c"]
    oh, ow = (h // 2, w // 2) if pool else (h, w)
    what = f"layernorm2d {nc.LN_IDS[nc.LN_RUNS.index((i, pool))]}"
    x = put(d["x"], s["x"])
    y = nan_view(n, oh, ow, c, s["y"])
    res = put(d["res"], s["res"]) if d["res"] is not None else None
    ops.layernorm2d(ctx, x, d["weight"].to(DEV), d["bias"].to(DEV), y, act=s["act"], alpha=s["alpha"], pool=pool,
                    res=res, eps=s["eps"])
    torch.cuda.synchronize()
    check_canary(y, what)
    unchanged(x, d["x"], what)
    got = y.v.cpu()
    check_bound(got, d, what)
    if s["values"] == "const":
        assert torch.equal(got, F.relu(d["bias"]) + d["res"]), f"{what}: not act(bias) + res bit for bit"


# ----------------------------------------------------------------------------- InstanceNorm / ADAIN
@pytest.mark.parametrize("i,form", nc.IN_RUNS, ids=nc.IN_IDS)
def test_instnorm_fp64(ctx, i, form):
    """s2v_instnorm_adain(_pad) against act((x - mean) * rsqrt(var + eps) * (1 + gamma) + beta) + res in
    float64, in the one-launch and in the two-launch form, each on its own: 1, 10 (250 live threads) and 64
    channel quads per block, a last channel block of one quad, the scalar kernels by channel count and by
    misalignment; planes from 1x1 to 70x40; gamma / beta absent or columns of one wider tensor; res absent or
    a slice.  The padded output is F.pad(y, (1, 1, 1, 1), 'reflect') of the kernel's own y, bit for bit, in a
    channel slice of a NaN-filled tensor: a 2-, 3- or k-row plane gets all of its border.

    Measured on MI355X: worst err / bound 0.206 fused (c260-33x31) and 0.235 in two launches (c260-70x40);
    the two forms give the same figures on every case that runs in both.  Before in_apply_v mirrored row 1
    of a 3-row plane (column 1 of a 3-column one) onto both borders, exactly the 18 padded runs with h == 3 or
    w == 3 failed here, each leaving 9 (3x3) or 7 (3x5, 5x3) NaN values per channel in the padded output."""
    d = nc.in_case(i)
    s = d["spec"]
    n, h, w, c = s["n"], s["h"], s["w"], s["c"]
    what = f"instnorm {s['name']} {form}"
    x = put(d["x"], s["x"])
    y = nan_view(n, h, w, c, s["y"])
    res = put(d["res"], s["res"]) if d["res"] is not None else None
    gamma = beta = None
    if s["gb"]:
        gb = d["gb"].to(DEV)
        gamma, beta = gb[:, :c], gb[:, c + 4:]
        assert gamma.stride(0) == 2 * c + 4
    pad = nan_view(n, h + 2, w + 2, c, s["pad"]) if s["pad"] is not None else None
    prev = ops.tune(ctx, ops.TUNE_IN_FUSED, h * w if form == "fused" else 0)
    try:
        ops.instnorm(ctx, x, y, gamma, beta, act=s["act"], alpha=s["alpha"], res=res, eps=s["eps"], pad_out=pad)
    finally:
        ops.tune(ctx, ops.TUNE_IN_FUSED, prev)
    torch.cuda.synchronize()
    check_canary(y, what)
    unchanged(x, d["x"], what)
    got = y.v.cpu()
    check_bound(got, d, what)
    if pad is not None:
        padded = pad.t.cpu()
        assert torch.isnan(padded[..., :4]).all() and torch.isnan(padded[..., 4 + c:]).all(), \
            f"{what}: the padded output wrote outside its channel slice"
        inside = padded[..., 4:4 + c]
        left = int(torch.isnan(inside).sum())
        assert left == 0, f"{what}: {left} of {inside.numel()} padded values were never written (still NaN)"
        want = F.pad(got.permute(0, 3, 1, 2), (1, 1, 1, 1), mode="reflect").permute(0, 2, 3, 1)
        assert torch.equal(inside, want), f"{what}: the padded output is not F.pad(y, 'reflect')"


# ----------------------------------------------------------------------------- resize
# NHWC views by case: (x view, y view); absent: dense on both sides
RESIZE_VIEWS = {"slices-by-size": ((16, 4), (16, 4)), "x2-c32-slice": ((32, 0), (40, 8))}


def resize_setup(i):
    """The device views of RESIZE_CASES[i]: the arguments of ops.resize before scale_factor / mode, the
    output tensor, and a function returning (result as NCHW on the CPU, everything else of the output)."""
    name, _, n, c, ih, iw = nc.RESIZE_CASES[i][:6]
    d = nc.resize_case(i, nc.RESIZE_CASES[i][8][0])
    oh, ow = d["oh"], d["ow"]
    xs = d["x"].permute(0, 2, 3, 1)                        # NHWC values
    if name == "nchw-to-nhwc":
        xt, x_off = d["x"].to(DEV), 0
        x_str = xt.stride()
    elif name == "nhwc-crop-to-nchw":
        t, l, fh, fw = nc.RESIZE_CROP
        xt = d["full"].permute(0, 2, 3, 1).contiguous().to(DEV)
        x_off, x_str = (t * fw + l) * c, (fh * fw * c, 1, fw * c, c)
    elif name.startswith("flip"):
        xt = xs.flip(2).contiguous().to(DEV)               # stored mirrored: the view reads it right to left
        x_off, x_str = (iw - 1) * c, (ih * iw * c, 1, iw * c, -c)
    elif name == "batch-stride":
        xt = torch.full((2 * n, ih, iw, c), NAN, device=DEV)
        xt[0::2] = xs.to(DEV)
        x_off, x_str = 0, (2 * ih * iw * c, 1, iw * c, c)
    else:
        xv = put(xs, RESIZE_VIEWS.get(name, ((c, 0), (c, 0)))[0])
        xt, x_off, x_str = xv.t, xv.coff, ops.nhwc_strides(xv)
    if name == "nhwc-crop-to-nchw":
        yt = torch.full((n, c, oh, ow), NAN, device=DEV)
        y_off, y_str = 0, yt.stride()

        def read():
            return yt.cpu(), torch.full((0,), NAN)
    else:
        yv = nan_view(n, oh, ow, c, RESIZE_VIEWS.get(name, ((c, 0), (c, 0)))[1])
        yt, y_off, y_str = yv.t, yv.coff, ops.nhwc_strides(yv)

        def read():
            t = yt.cpu()
            inside = torch.zeros(yv.cs, dtype=torch.bool)
            inside[yv.coff:yv.coff + c] = True
            return t[..., inside].permute(0, 3, 1, 2), t[..., ~inside]
    return d, (xt, x_off, (n, c, ih, iw), x_str, yt, y_off, (oh, ow), y_str), yt, read


@pytest.mark.parametrize("i,mode", nc.RESIZE_RUNS, ids=nc.RESIZE_IDS)
def test_resize_fp64(ctx, i, mode):
    """s2v_resize in both modes through its three kernels: NCHW -> NHWC and a cropped NHWC -> NCHW copy at
    scale 1 (bit-exact), sources read right to left through a negative x stride (generic and float4), channel
    slices on both sides, scale_factor 0.5 and 3, every second image of a batch, 1x1 and 1x9 sources, exact x2
    (the 2x2-quad kernel bit-equal to the generic float4 kernel), and row counts past the 65535 grid rows of
    the x2 and of the float4 kernel.  Bilinear against float64 taps with torch's float32 coordinates, nearest
    bit-equal to F.interpolate(mode='nearest').

    Measured on MI355X: err <= 0.11 tol on every bilinear case (1.0e-07 absolute at the most; e_ref 5e-08 to
    1.3e-07).  The x2 / float4 bit-equality failed on all four x2 cases (by an ulp, both within 0.11 tol)
    until the three kernels took their four-tap sum from one function with its fmas written out."""
    name, kernel = nc.RESIZE_CASES[i][:2]
    d, args, yt, read = resize_setup(i)
    d = nc.resize_case(i, mode)
    what = f"resize {nc.RESIZE_IDS[nc.RESIZE_RUNS.index((i, mode))]}"
    results = []
    for up2 in ((1, 0) if kernel == "x2" and mode == 0 else (None,)):
        yt.fill_(NAN)
        prev = ops.tune(ctx, ops.TUNE_RESIZE_UP2, up2) if up2 is not None else None
        try:
            ops.resize(ctx, *args, scale_factor=d["sf"], mode=mode)
        finally:
            if up2 is not None:
                ops.tune(ctx, ops.TUNE_RESIZE_UP2, prev)
        torch.cuda.synchronize()
        got, beside = read()
        tag = what if up2 is None else f"{what} up2={up2}"
        assert torch.isnan(beside).all(), f"{tag}: wrote outside its channel slice"
        left = int(torch.isnan(got).sum())
        assert left == 0, f"{tag}: {left} output values are NaN (never written, or read from a canary)"
        if mode == 1:
            assert torch.equal(got, d["exact"]), f"{tag}: differs from F.interpolate(mode='nearest')"
        else:
            err = (got.double() - d["ref64"]).abs()
            worst = int(torch.argmax(err))
            at = tuple(int(k) for k in np.unravel_index(worst, tuple(err.shape)))
            e = float(err.max())
            print(f"{tag}: e_ref={d['e_ref']:.2e} floor={d['floor']:.2e} tol={d['tol']:.2e} err={e:.2e} "
                  f"({e / d['tol']:.3f} tol) at {at}")
            assert e <= d["tol"], f"{tag}: element {at}: err {e:.3e} = {e / d['tol']:.2f} x tol {d['tol']:.3e}"
            if name == "nhwc-crop-to-nchw":
                assert torch.equal(got, d["x"]), f"{tag}: a copy at scale 1 must be bit-exact"
        results.append(got)
    if len(results) == 2:
        assert torch.equal(results[0], results[1]), f"{what}: the x2 kernel differs from the generic float4 kernel"


# ----------------------------------------------------------------------------- pad_reflect
@pytest.mark.parametrize("li,pi", nc.PAD_RUNS, ids=nc.PAD_IDS)
def test_pad_reflect_exact(ctx, li, pi):
    """s2v_pad_reflect bit-equal to F.pad(mode='reflect'): asymmetric pads, the largest legal pad (dim - 1),
    no pad at all and the FFC's (1, 1, 1, 1), through the scalar kernel (c = 3, and c = 8 misaligned) and the
    float4 kernel (dense, and slices of wider tensors on both sides)."""
    name, c, xv, yv, _ = nc.PAD_LAYOUTS[li]
    d = nc.pad_case(li, pi)
    n, oh, ow, _ = d["exact"].shape
    what = f"pad_reflect {nc.PAD_IDS[nc.PAD_RUNS.index((li, pi))]}"
    x = put(d["x"], xv)
    y = nan_view(n, oh, ow, c, yv)
    ops.pad_reflect(ctx, x, y, nc.PAD_PADS[pi])
    torch.cuda.synchronize()
    check_canary(y, what)
    unchanged(x, d["x"], what)
    assert torch.equal(nc.bits(y.v.cpu()), nc.bits(d["exact"])), what


# ----------------------------------------------------------------------------- row_pack
@pytest.mark.parametrize("i", range(len(nc.PACK_CASES)), ids=[c[0] for c in nc.PACK_CASES])
def test_row_pack_exact(ctx, i):
    """s2v_row_pack bit-equal to a plain index loop, +0.0 outside the row and in channels [kw * c, ycs) of an
    output that held NaN: 7-tap packing of 3 and 6 channels, 3 taps without left padding, a row narrower than
    the filter, inputs that are slices of a wider pitch."""
    name, n, h, w, c, kw, pw, ycs, xv = nc.PACK_CASES[i]
    d = nc.pack_case(i)
    x = put(d["x"], xv)
    y = nan_view(n, h, w, ycs, (ycs, 0))
    ops.row_pack(ctx, x, y, kw, pw)
    torch.cuda.synchronize()
    got = y.t.cpu()
    unchanged(x, d["x"], f"row_pack {name}")
    wrong = nc.bits(got) != nc.bits(d["exact"])
    assert not wrong.any(), (f"row_pack {name}: {int(wrong.sum())} values differ, first at "
                             f"{tuple(int(k) for k in wrong.nonzero()[0])}")


# ----------------------------------------------------------------------------- rejections
def all_nan(*views):
    torch.cuda.synchronize()
    return all(bool(torch.isnan(v.t).all()) for v in views)


def test_rejected_calls_raise_and_write_nothing(ctx):
    """pad_out on the scalar path (c % 4 != 0, a misaligned x, a misaligned pad_out), a reflect pad >= the
    dimension, a row_pack pitch that is no multiple of 4 (or a sliced output), and a pooled LayerNorm2d of a
    one-row image are errors, raised before anything is launched: every output still holds its NaN fill."""
    n, h, w = 2, 4, 5
    for c, xv, yv, pv in ((6, (6, 0), (6, 0), (6, 0)), (8, (12, 2), (8, 0), (8, 0)), (8, (8, 0), (8, 0), (12, 2))):
        x = put(nc.rand(n, h, w, c, seed=7000), xv)
        y, pad = nan_view(n, h, w, c, yv), nan_view(n, h + 2, w + 2, c, pv)
        with pytest.raises(RuntimeError, match="instnorm_pad"):
            ops.instnorm(ctx, x, y, pad_out=pad)
        assert all_nan(y, pad), "a refused instnorm wrote"
        ops.instnorm(ctx, x, y)                              # the same views without pad_out are fine
        assert not all_nan(y)
    x = put(nc.rand(n, h, w, 8, seed=7001), (8, 0))
    for pads in ((h, 0, 0, 0), (0, h, 0, 0), (0, 0, w, 0), (0, 0, 0, w + 1)):
        y = nan_view(n, h + pads[0] + pads[1], w + pads[2] + pads[3], 8, (8, 0))
        with pytest.raises(RuntimeError, match="padding must be < input size"):
            ops.pad_reflect(ctx, x, y, pads)
        assert all_nan(y), "a refused pad_reflect wrote"
    x = put(nc.rand(n, h, w, 3, seed=7002), (3, 0))
    for yv, c in (((22, 0), 22), ((24, 0), 21), ((28, 4), 24)):      # 22 floats; 24 but a view of 21; a slice
        y = nan_view(n, h, w, c, yv)
        with pytest.raises(RuntimeError, match="row_pack"):
            ops.row_pack(ctx, x, y, 7, 3)
        assert all_nan(y), "a refused row_pack wrote"
    wgt, bias = torch.ones(8, device=DEV), torch.zeros(8, device=DEV)
    for hh, ww in ((1, 4), (4, 1)):
        x = put(nc.rand(1, hh, ww, 8, seed=7003), (8, 0))
        y = nan_view(1, max(hh // 2, 1), max(ww // 2, 1), 8, (8, 0))
        with pytest.raises(RuntimeError, match="layernorm2d"):
            ops.layernorm2d(ctx, x, wgt, bias, y, pool=True)
        assert all_nan(y), "a refused layernorm2d wrote"


def test_resize_refuses_views_that_leave_their_tensor(ctx):
    """A negative stride is legal only with an offset that keeps the view inside its tensor: the flipped view
    without its row-end offset starts before the data and is refused, as is one past the end."""
    n, c, ih, iw = 1, 4, 3, 5
    xt = torch.zeros(n, ih, iw, c, device=DEV)
    y = nan_view(n, ih, iw, c, (c, 0))
    args = ((n, c, ih, iw), (ih * iw * c, 1, iw * c, -c), y.t, 0, (ih, iw), ops.nhwc_strides(y))
    for off in (0, (iw - 2) * c, ih * iw * c):
        with pytest.raises(RuntimeError, match="leaves its tensor"):
            ops.resize(ctx, xt, off, *args)
    assert all_nan(y)
    ops.resize(ctx, xt, (iw - 1) * c, *args)
    assert not all_nan(y)
