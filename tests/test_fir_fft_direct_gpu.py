"""Direct fp64 parity of the FIR resampler of csrc/fir.hip (``ops.fir2d``: fir2d_blur4_rows and the up2, down2,
runtime-generic and scalar instantiations of fir2d_kernel), of the GPEN plane kernel behind
``torch_ops.upfirdn2d`` (csrc/misc.hip) and of the separable real DFTs of csrc/fft.hip (``ops.rfft2`` /
``ops.irfft2``: the MFMA kernels at 12 / 24 / 48 and the generic LDS kernels), each kernel called on its own
at the shapes, views and value sets where it can go wrong.  tests/fir_fft_cases.py builds the inputs, the
float64 references and the per-element bounds on the CPU; tests/test_fir_fft_cases_host.py checks there that
the cases reach the kernels they are listed for and that the bounds tell a wrong kernel from a right one.

Every output is a channel slice of a NaN-filled tensor or a NaN-filled tensor between NaN guard bands, every
channel beside a sliced input holds NaN: what a kernel must write has to come out finite, what it must not
touch has to keep its NaN, what it must not read would show in the result, and the input is unchanged
afterwards.  Run with ``-s`` for the achieved err / bound of every case and the CPU float32 figure beside it.

K_FIR = 8, K_FFT = 16 (fir_fft_cases' docstring; the CPU float32 evaluations use at most half the bound).
Worst err / bound measured on MI355X, all 121 tests passing with the kernels as they were (no kernel change
was needed):
  fir2d    blur4_rows 0.305, up2 0.256, down2 0.211, runtime-generic 0.278, scalar 0.272 (CPU float32 0.364,
           0.256, 0.211, 0.285, 0.272); the exact set and every float4 / scalar pair bit for bit
  plane    upfirdn2d_plane4 0.486, upfirdn2d_kernel 0.394 (the CPU float32 figures are the same: 0.486, 0.394)
  rfft2    MFMA 0.261, generic 0.147;  irfft2  MFMA 0.257, generic 0.262 (offset set; CPU float32 the same to
           three digits: the chains are the CPU's); unit set <= 0.101, impulse set <= 0.135

Sensitivity (arithmetic-only edits to a scratch copy of csrc/fir.hip / csrc/fft.hip, built and run against
these tests on an MI355X, nothing of it kept):
  the filter not flipped (``ks[i] = k[i]`` in both fir kernels)     all 52 random-filter fir2d cases fail (err /
      bound 1.7e6 .. 2.1e7); the 4 exact-set cases pass, their GPEN filter being symmetric
  pad_y0 / pad_x0 swapped in the three fir launches                 the 36 fir2d cases with py0 != px0 fail (err /
      bound >= 1.4e6), the 20 others pass
  ``+fi`` for ``-fi`` in the forward H pass (both rfft2 kernels)    42 of the 51 FFT runs fail in rfft2 (err / bound
      946 .. 2.1e6); the 9 that pass have no imaginary part to get wrong: H = 1, W = 2, and the n = 1 impulses,
      which sit in row 0
  the imaginary half stored at ``o[scs / 2]`` for ``o[C]``          the 27 runs with pitch 2C + 8 fail ("wrote into
      the padding channels of its pitch"), the 24 with pitch 2C pass
"""
import math

import numpy as np
import pytest
import torch

import s2v_import  # noqa: F401

pytestmark = pytest.mark.gpu

import fir_fft_cases as fc  # noqa: E402
from s2v_amd import ops, torch_ops  # noqa: E402
from s2v_amd.ops import NHWC  # noqa: E402

DEV = "cuda"
NAN = float("nan")
NAN_BITS = int(torch.tensor(NAN, dtype=torch.float32).view(torch.int32))
GUARD = 1024                                   # floats before and after a banded output (16-byte aligned)


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


def all_nan(*tensors):
    torch.cuda.synchronize()
    return all(bool(torch.isnan(t).all()) for t in tensors)


class Banded:
    """A NaN-filled device tensor of ``shape`` between two NaN-filled guard bands."""

    def __init__(self, *shape):
        numel = math.prod(shape)
        self.flat = torch.full((GUARD + numel + GUARD,), NAN, device=DEV)
        self.t = self.flat[GUARD:GUARD + numel].view(shape)

    def check(self, what, c):
        """The guard bands and the channels >= c of the pitch still hold the NaN they were filled with; the
        channels below c are finite."""
        bits = self.flat.view(torch.int32)
        assert bool((bits[:GUARD] == NAN_BITS).all()), f"{what}: wrote before its output"
        assert bool((bits[-GUARD:] == NAN_BITS).all()), f"{what}: wrote behind its output"
        if c < self.t.shape[-1]:
            assert bool((self.t[..., c:].contiguous().view(torch.int32) == NAN_BITS).all()), \
                f"{what}: wrote into the padding channels of its pitch"
        left = int(torch.isnan(self.t[..., :c]).sum())
        assert left == 0, f"{what}: {left} output values are NaN (never written, or computed from a canary)"
        assert bool(torch.isfinite(self.t[..., :c]).all()), f"{what}: non-finite output"


def check_bound(got, ref64, bound, cpu32, what) -> float:
    """Every element within its own bound; prints the worst ratio and the CPU float32 evaluations' beside it."""
    err = (got.double() - ref64).abs()
    ratio = err / bound
    worst = int(torch.argmax(torch.nan_to_num(ratio, nan=float("inf"))))
    at = tuple(int(k) for k in np.unravel_index(worst, tuple(ratio.shape)))
    r = float(ratio.flatten()[worst])
    cpu = max(float(((t.double() - ref64).abs() / bound).max()) for t in cpu32)
    print(f"{what}: max err={float(err.max()):.2e} worst err / bound={r:.3f} at {at} (CPU float32 {cpu:.3f})")
    assert r <= 1.0, (f"{what}: element {at}: got {float(got[at])!r}, reference {float(ref64[at])!r}, "
                      f"err / bound = {r:.3f}")
    return r


# ----------------------------------------------------------------------------- fir2d
def run_fir(ctx, d, xview, yview, bias_offset, what):
    s = d["spec"]
    x = put(d["x"], xview)
    y = nan_view(s["n"], s["oh"], s["ow"], s["c"], yview)
    bias = None
    if d["bias"] is not None:
        bias = d["bias_full"].to(DEV)[1:1 + s["c"]] if bias_offset else d["bias"].to(DEV)
        assert bias.is_contiguous() and (bias.data_ptr() % 16 != 0) == bias_offset
    ops.fir2d(ctx, x, d["k"].to(DEV), y, up=s["up"], down=s["down"], pad0=s["pad0"], gain=s["gain"], bias=bias,
              act=s["act"], alpha=s["alpha"], post=s["post"])
    torch.cuda.synchronize()
    check_canary(y, what)
    unchanged(x, d["x"], what)
    return y.v.cpu()


@pytest.mark.parametrize("i", range(len(fc.FIR_CASES)), ids=fc.FIR_IDS)
def test_fir2d_fp64(ctx, i):
    """s2v_fir2d against upfirdn2d in float64 with the fused epilogue, per element within K_FIR * 2^-24 * post *
    (|gain| * sum|x k| + |bias|): random asymmetric filters, asymmetric and negative pads, outputs larger than
    upfirdn2d's own; fir2d_blur4_rows at output heights below a strip and at every remainder of it, widths 1
    and 2, dense and as slices (16, 4) -> (20, 8); the up2 and down2 instantiations; the runtime-generic
    float4 kernel with 3x3 .. 8x8 filters, up 3, up 2 / down 2 and up 2 / down 3; the scalar kernel by channel
    count and by a misaligned x, y or bias; no epilogue, and gain 1.5 / post sqrt(2) / bias with each
    activation.  The exact set equals the float64 reference bit for bit.  Every float4 case runs again from a
    misaligned copy of its input, which takes the scalar kernel: the two results are the same bits (fir.hip's
    claim for the strip form, held for every float4 form).

    Measured on MI355X: worst err / bound 0.305 (blur4-sym-6x10-p2.2-o7x11, 1.2e-06 absolute; the CPU float32
    evaluations reach 0.364 there); per kernel in the module docstring."""
    d = fc.fir_case(i)
    s = d["spec"]
    what = f"fir2d {s['name']}"
    got = run_fir(ctx, d, s["x"], s["y"], s["bias"] == "offset", what)
    check_bound(got, d["ref64"], fc.fir_bound(d), (d["conv32"], d["fma32"]), what)
    if s["values"] == "exact":
        assert torch.equal(got.double(), d["ref64"]), f"{what}: the exact set differs from the float64 reference"
    if s["kernel"] != "scalar":
        other = run_fir(ctx, d, (s["c"] + 4, 2), s["y"], False, what + " (scalar kernel)")
        differ = fc.bits(got) != fc.bits(other)
        assert not differ.any(), (f"{what}: {int(differ.sum())} values of the float4 kernel are not the scalar "
                                  f"kernel's bits, first at {tuple(int(k) for k in differ.nonzero()[0])}")


def test_fir2d_rejections(ctx):
    """A filter of 65 taps, up = 0 and down = 0 raise before anything is launched: the output keeps its NaN."""
    x = put(fc.rand(2, 6, 7, 8, seed=8900), (8, 0))
    for k, up, down, match in ((torch.ones(5, 13), 1, 1, "1..64 taps"), (torch.ones(4, 4), 0, 1, "up/down"),
                               (torch.ones(4, 4), 1, 0, "up/down")):
        y = nan_view(2, 6, 7, 8, (8, 0))
        with pytest.raises(RuntimeError, match=match):
            ops.fir2d(ctx, x, k.to(DEV), y, up=up, down=down, pad0=(1, 1))
        assert all_nan(y.t), "a refused fir2d wrote"
    y = nan_view(2, 6, 7, 8, (8, 0))
    ops.fir2d(ctx, x, torch.ones(8, 8, device=DEV), y, pad0=(3, 3))          # 64 taps are fine
    assert not all_nan(y.t)


# ----------------------------------------------------------------------------- the GPEN plane kernel
@pytest.mark.parametrize("i", range(len(fc.PLANE_CASES)), ids=[c[0] for c in fc.PLANE_CASES])
def test_upfirdn2d_plane_fp64(i):
    """torch_ops.upfirdn2d on NCHW float32 (upfirdn2d_plane4: a 16 x 64 output tile per block) against the same
    float64 reference, within K_FIR * 2^-24 * sum|x k|: outputs of 16 and 17 rows, 64 and 65 columns in the
    blur, up2 and down2 forms, a random filter, asymmetric pads; a negative first pad takes upfirdn2d_kernel
    and is held to the same bound.

    Measured on MI355X: worst err / bound 0.486 (down2-negp1-16x65, 7.5e-07 absolute), the figure of the CPU
    fma chain: the kernel's fmas are that chain.  0.394 through upfirdn2d_kernel (blur-neg-17x65)."""
    name = fc.PLANE_CASES[i][0]
    _, _, up, down, pad, h, w = fc.PLANE_CASES[i]
    d = fc.plane_case(i)
    x = d["x"].to(DEV)
    got = torch_ops.upfirdn2d(x, d["k"].to(DEV), up=up, down=down, pad=pad)
    torch.cuda.synchronize()
    assert tuple(got.shape) == tuple(d["ref64"].shape), name
    assert torch.equal(x.cpu(), d["x"]), f"{name}: the input changed"
    got = got.cpu()
    assert torch.isfinite(got).all(), name
    check_bound(got, d["ref64"], fc.fir_bound(d), (d["conv32"], d["fma32"]), f"upfirdn2d {name}")


# ----------------------------------------------------------------------------- rfft2 / irfft2
def run_rfft2(ctx, d, what):
    s = d["spec"]
    n, c, h, w = s["n"], s["c"], s["h"], s["w"]
    x = put(d["x"], s["x"])
    spec = Banded(n, h * (w // 2 + 1), s["scs"])
    ops.rfft2(ctx, x, ops.fft_tables(h, w, DEV), spec.t)
    torch.cuda.synchronize()
    spec.check(what, 2 * c)
    unchanged(x, d["x"], what)
    return spec.t[..., :2 * c].cpu()


def run_irfft2(ctx, d, what):
    s = d["spec"]
    n, c, h, w = s["n"], s["c"], s["h"], s["w"]
    sp = torch.full((n, h * (w // 2 + 1), s["scs"]), NAN, device=DEV)
    sp[..., :2 * c] = d["sp"].to(DEV)
    y = nan_view(n, h, w, c, s["y"])
    res = put(d["res"], s["res"]) if d["res"] is not None else None
    ops.irfft2(ctx, sp, ops.fft_tables(h, w, DEV), y, res)
    torch.cuda.synchronize()
    check_canary(y, what)
    assert torch.equal(sp[..., :2 * c].cpu(), d["sp"]) and bool(torch.isnan(sp[..., 2 * c:]).all()), \
        f"{what}: the spectrum changed"
    if res is not None:
        unchanged(res, d["res"], what)
    return y.v.cpu()


@pytest.mark.parametrize("i,values", fc.FFT_RUNS, ids=fc.FFT_IDS)
def test_rfft2_irfft2_fp64(ctx, i, values):
    """s2v_rfft2 and s2v_irfft2 against the two separable passes in float64 on the kernels' own float32
    tables, per element within K_FFT * 2^-24 * B (B: the passes on absolute values): the MFMA kernels at 12,
    24 and 48 with 3, 8 and 16 images and 1, 2 and 3 channel groups (n in {8, 16}: the XCD permutation of
    fft_block), the generic kernels at W != H, odd sizes, H = 1, W = 2, 24 x 12, two groups per image, and
    at 40 x 56 / 56 x 56 (100 / 142 KB of dynamic LDS); x dense and a slice, spectrum pitch 2C and 2C + 8 (the
    imaginary half at + C, the 8 channels behind keep their NaN), irfft2 without res, with a dense one and
    with a (C + 5, 2) slice, y dense and a (C + 3, 1) slice; U[-1, 1), 30 + U[-0.5, 0.5) and one impulse per
    (image, channel) whose position and amplitude name the pair.

    Measured on MI355X: worst err / bound 0.261 forward (mf48-n8-c8-offset) and 0.262 inverse (g40x56-offset),
    each the figure of the CPU fma chain; the unit set stays below 0.101, the impulse set below 0.135."""
    d = fc.fft_case(i, values)
    what = fc.FFT_IDS[fc.FFT_RUNS.index((i, values))]
    got = run_rfft2(ctx, d, f"rfft2 {what}")
    check_bound(got, d["spec64"], fc.fft_bound(d["spec_unit"]), (d["spec_mm32"], d["spec_fma32"]), f"rfft2 {what}")
    got = run_irfft2(ctx, d, f"irfft2 {what}")
    check_bound(got, d["y64"], fc.fft_bound(d["y_unit"]), (d["y_mm32"], d["y_fma32"]), f"irfft2 {what}")


def test_fft_rejections(ctx):
    """C % 4 != 0, a 64 x 64 tile (which does not fit in LDS: the message says so), w = 1, a spectrum narrower
    than 2C and, for rfft2, an x whose pitch is no multiple of 4 raise before anything is launched: every
    output keeps its NaN."""
    def attempt(n, h, w, c, match, *, xview=None, scs=None, inverse=True):
        wf = w // 2 + 1
        scs = 2 * c if scs is None else scs
        tables = ops.fft_tables(h, w, DEV)
        x = put(fc.rand(n, h, w, c, seed=8950), xview or (c, 0))
        spec = torch.full((n, h * wf, scs), NAN, device=DEV)
        with pytest.raises(RuntimeError, match=match):
            ops.rfft2(ctx, x, tables, spec)
        assert all_nan(spec), f"a refused rfft2 wrote ({match})"
        if inverse:
            sp = torch.zeros(n, h * wf, scs, device=DEV)
            y = nan_view(n, h, w, c, (c, 0))
            with pytest.raises(RuntimeError, match=match):
                ops.irfft2(ctx, sp, tables, y)
            assert all_nan(y.t), f"a refused irfft2 wrote ({match})"

    attempt(2, 6, 10, 6, "C % 4 != 0", xview=(8, 0), scs=12)
    attempt(1, 64, 64, 4, "64x64 tile does not fit in LDS")
    attempt(2, 5, 1, 4, "bad args")
    attempt(2, 6, 10, 8, ">= 2C", scs=12)
    attempt(2, 6, 10, 4, "pitches", xview=(6, 0), inverse=False)
    # the accepted neighbours run
    x = put(fc.rand(2, 6, 10, 4, seed=8951), (8, 0))
    spec = torch.full((2, 36, 8), NAN, device=DEV)
    ops.rfft2(ctx, x, ops.fft_tables(6, 10, DEV), spec)
    assert not all_nan(spec)
