"""LNet's fused FFC kernels (csrc/ffc.hip: ffc_spec_fwd / ffc_spec_inv / ffc_norm) against plain float64
references of the operations they compute, at all three levels (12 / 24 / 48) in both split-precision
arithmetics, in every argument form the entry points accept (tests/ffc_cases.py builds the operands,
references and tolerances; tests/test_ffc_cases_host.py checks them on the CPU).

Every output is allocated inside a larger NaN-filled buffer: what a kernel must write has to come out finite,
the guard band before and after it and the padding channels of a wide pitch keep their NaN bit pattern.
Run with ``-s`` to see the worst err / tol of every case.

Worst err / tol measured on MI355X, f16x3 / bf16x3 at levels 12, 24, 48:
  spec_fwd t1    random 0.041/0.017, 0.048/0.039, 0.048/0.045; exact set bit for bit
  spec_fwd spec  0.180/0.188, 0.224/0.239, 0.250/0.281 (transform rule, both sets)
  spec_inv u     exact 0.143, 0.211, 0.231 in both (transform rule); random 0.002/0.001, 0.004/0.001, 0.004/0.001
  norm l / g     random l 0.038, 0.032, 0.033, g 0.010/0.008, 0.008/0.013, 0.008/0.019; exact l 0.031, g 0.050
The propagated bound of the random inv set is a worst case (every frequency's GEMM error at its bound and in
phase): it sits ~250x above the measured error, and it is the exact set that holds the inverse transform and
the + t1 residual to fp32.  The split-precision GEMM code (ffc_strip_gemm) is shared by the three kernels and is
held to the GEMM rule through t1 and through the g channels of the norm.

Sensitivity (arithmetic-only changes to a scratch copy of csrc/ffc.hip, each failing these tests): dropping the
a_lo * b_hi MFMA term fails spec_fwd t1 (err / tol 5 .. 26) and the norm's g channels (2.5 .. 8.6); the sign of
-fi / -gi in the forward / inverse H pass fails spec_fwd spec / spec_inv u; gamma for 1 + gamma and the unbiased
variance fail the norm (l and g channels); dropping + t1 fails spec_inv u.
"""
import contextlib
import math

import pytest
import torch

import s2v_import  # noqa: F401

pytestmark = pytest.mark.gpu

import ffc_cases as fc  # noqa: E402
from s2v_amd import ops, torch_ops  # noqa: E402
from s2v_amd.ops import NHWC, ConvW  # noqa: E402

DEV = "cuda"
NAN = float("nan")
NAN_BITS = int(torch.tensor(NAN, dtype=torch.float32).view(torch.int32))
GUARD = 1024                                   # floats before and after every output (16-byte aligned)
PRECS = ("f16x3", "bf16x3")


@pytest.fixture
def ctx():
    return ops.Ctx(DEV)


@contextlib.contextmanager
def arithmetic(prec):
    """ops.set_precision(prec) for the launches of one test."""
    prev = ops.set_precision(prec)
    try:
        yield prec
    finally:
        ops.set_precision(prev)


# level outermost, arithmetic innermost: both arithmetics of a level share its cached references
per_level = pytest.mark.parametrize("h", fc.LEVELS)
per_prec = pytest.mark.parametrize("prec", PRECS)


class Banded:
    """A NaN-filled device tensor of ``shape`` between two NaN-filled guard bands."""

    def __init__(self, *shape):
        numel = math.prod(shape)
        self.flat = torch.full((GUARD + numel + GUARD,), NAN, device=DEV)
        self.t = self.flat[GUARD:GUARD + numel].view(shape)

    def check(self, what, c=None):
        """The guard bands (and the channels >= c of a wide pitch) still hold the NaN they were filled with."""
        bits = self.flat.view(torch.int32)
        assert bool((bits[:GUARD] == NAN_BITS).all()), f"{what}: wrote before its output"
        assert bool((bits[-GUARD:] == NAN_BITS).all()), f"{what}: wrote behind its output"
        if c is not None and c < self.t.shape[-1]:
            assert bool((self.t[..., c:].contiguous().view(torch.int32) == NAN_BITS).all()), \
                f"{what}: wrote into the padding channels of its pitch"


def wide(values: torch.Tensor, pitch: int, off: int = 0) -> NHWC:
    """``values`` [n, h, w, c] as channels [off, off + c) of a NaN-filled [n, h, w, pitch] device tensor."""
    n, h, w, c = values.shape
    t = torch.full((n, h, w, pitch), NAN, device=DEV)
    t[..., off:off + c] = values.to(DEV)
    return NHWC(t, off, c)


def conv_w(w, scale, shift) -> ConvW:
    """A 1x1 ConvW whose folded scale / shift are exactly the case's (bn_eps 0), or absent."""
    bn = None if scale is None else fc.bn_tuple(scale, shift)
    cw = ConvW(w, None, DEV, bn=bn, bn_eps=0.0)
    assert (cw.scale is None) == (scale is None) and (cw.shift is None) == (scale is None)
    if scale is not None:
        assert torch.equal(cw.scale.cpu(), scale) and torch.equal(cw.shift.cpu(), shift)
    return cw


def worst(err: torch.Tensor, tol) -> float:
    return float((err / tol).max())


# ----------------------------------------------------------------------------- runners
def run_fwd(ctx, cw, L, x, xf, x_scale=None):
    """ffc_spec_fwd on x [n, H, H, cg] (host) -> (t1 [n, H, H, cc], spec [n, F, 2cc]) on the host.
    x_scale: call the raw op with that activation pre-scale instead of ops.ffc_spec_fwd."""
    n, h = x.shape[0], L.h
    xv = wide(x, L.c + 8, L.cl) if xf == "wide" else NHWC(x.contiguous().to(DEV))
    t1, spec = Banded(n, h, h, L.cc), Banded(n, L.f, 2 * L.cc)
    tables = ops.fft_tables(h, h, DEV)
    if x_scale is None:
        ops.ffc_spec_fwd(ctx, xv, cw, tables, NHWC(t1.t), spec.t)
    else:
        pc = ops.prec_code()
        torch_ops.load()
        torch.ops.s2v.ffc_spec_fwd_(xv.v, cw.wt_x3(ctx, pc), cw.split_scale(pc), x_scale, cw.scale, cw.shift, tables,
                                    t1.t, spec.t, None, pc)
    torch.cuda.synchronize()
    t1.check("ffc_spec_fwd t1")
    spec.check("ffc_spec_fwd spec")
    return t1.t.cpu(), spec.t.cpu()


def check_fwd(d, got, prec, what):
    t1, spec = got
    assert torch.isfinite(t1).all() and torch.isfinite(spec).all(), f"{what}: output not completely written"
    r_t1 = worst((t1.double() - d["t1"]).abs(), fc.gemm_tol(d["bound"], prec))
    # the kernel transforms exactly the t1 it stores: no GEMM term in the spectrum's tolerance
    r_spec = worst((spec.double() - fc.rfft64(t1)).abs(), d["tol_t"])
    print(f"{what}: t1 err/tol {r_t1:.3f}, spec err/tol {r_spec:.3f} (tol_T {d['tol_t']:.2e})")
    assert r_t1 <= 1.0, f"{what}: t1 err / tol = {r_t1:.3f}"
    assert r_spec <= 1.0, f"{what}: spec err / tol_T = {r_spec:.3f}"
    if d.get("kind") == "exact":
        assert torch.equal(t1.double(), d["t1"]), f"{what}: exact-set t1 differs from the reference"
    return r_t1, r_spec


def run_inv(ctx, cw, L, spec, t1):
    n, h = spec.shape[0], L.h
    u = Banded(n, h, h, L.cc)
    ops.ffc_spec_inv(ctx, spec.contiguous().to(DEV), cw, ops.fft_tables(h, h, DEV), NHWC(t1.contiguous().to(DEV)),
                     NHWC(u.t))
    torch.cuda.synchronize()
    u.check("ffc_spec_inv u")
    return u.t.cpu()


def check_inv(d, u, prec, what):
    assert torch.isfinite(u).all(), f"{what}: u not completely written"
    tol = d["tol_t"] if d["kind"] == "exact" else fc.inv_tol(d, prec)
    r = worst((u.double() - d["u"]).abs(), tol)
    print(f"{what}: u err/tol {r:.3f} ({d['kind']} set, tol_T {d['tol_t']:.2e})")
    assert r <= 1.0, f"{what}: u err / tol = {r:.3f}"
    return r


def run_norm(ctx, cw, d, *, pad="case", act=None, y=None, u=None, gamma="case", beta="case", out_extra=None):
    """ffc_norm in the argument form of the norm case d -> (out [n, H, H, C], pad [n, H+2, H+2, C] or None)
    on the host.  pad=None: the same run without pad_out; y / u: other operand values."""
    L, n, h = d["level"], d["n"], d["level"].h
    c = L.c
    yval = d["yv"] if y is None else y
    out = Banded(n, h, h, c + (d["out"] if out_extra is None else out_extra))
    outv = NHWC(out.t, 0, c)
    if d["y"] == "out":
        out.t[..., :c] = yval.to(DEV)
        yv = outv
    else:
        yv = wide(yval, c + d["y"])
    resv = None
    if d["res"] == "out":
        out.t[..., :c] = d["resv"].to(DEV)
        resv = outv
    elif d["res"] is not None:
        resv = wide(d["resv"], c + d["res"])
    g = b = None
    if d["gb"] == "halves":
        gb = torch.cat([d["gamma"], d["beta"]], 1).to(DEV)
        g, b = gb[:, :c], gb[:, c:]
    elif d["gb"] == "dense":
        g, b = d["gamma"].to(DEV), d["beta"].to(DEV)
    g = g if isinstance(gamma, str) else gamma
    b = b if isinstance(beta, str) else beta
    pad_extra = d["pad"] if pad == "case" else pad
    padb = None if pad_extra is None else Banded(n, h + 2, h + 2, c + pad_extra)
    ops.ffc_norm(ctx, yv, NHWC((d["u"] if u is None else u).contiguous().to(DEV)), cw, outv, g, b,
                 act=fc.ACTS[d["act"]] if act is None else act, alpha=fc.ALPHA, res=resv, eps=d["eps"],
                 pad_out=None if padb is None else NHWC(padb.t, 0, c))
    torch.cuda.synchronize()
    out.check("ffc_norm out", c)
    if padb is not None:
        padb.check("ffc_norm pad_out", c)
    return out.t[..., :c].cpu(), None if padb is None else padb.t[..., :c].cpu()


def check_norm(d, out, tol, what):
    cl = d["level"].cl
    assert torch.isfinite(out).all(), f"{what}: out not completely written"
    ratio = (out.double() - d["ref"]).abs() / tol
    r_l, r_g = float(ratio[..., :cl].max()), float(ratio[..., cl:].max())
    print(f"{what}: out err/tol l channels {r_l:.3f}, g channels {r_g:.3f} ({d['kind']} set)")
    assert r_l <= 1.0, f"{what}: l channels err / tol = {r_l:.3f} (g channels {r_g:.3f})"
    assert r_g <= 1.0, f"{what}: g channels err / tol = {r_g:.3f} (l channels {r_l:.3f})"
    return r_l, r_g


# ----------------------------------------------------------------------------- the three kernels
@per_level
@per_prec
def test_ffc_spec_fwd_fp64(ctx, prec, h):
    """t1 against relu((x_g W1^T) * scale + shift) in float64 by the GEMM rule, bit for bit on the exact set;
    spec against rfftn of the t1 the kernel stored by the transform rule; x_g dense and as a channel slice
    at offset cl of a wider tensor, scale / shift present (negative scales) and absent, n = 3 / 16 (/ 8)."""
    with arithmetic(prec):
        for i, c in enumerate(fc.FWD_CASES):
            if c.get("only", h) != h:
                continue
            d = fc.fwd_case(h, i)
            got = run_fwd(ctx, conv_w(d["w"], d["scale"], d["shift"]), d["level"], d["x"], d["xf"])
            ctx.check_range()
            check_fwd(d, got, prec, f"spec_fwd {h} {prec} {c['name']}")


@per_level
@pytest.mark.parametrize("x_scale", fc.X_SCALES)
@per_prec
def test_ffc_spec_fwd_explicit_x_scale(ctx, prec, h, x_scale):
    """The raw op with an activation pre-scale of 2^-3 / 2^4 and the input scaled the other way: the epilogue
    undoes it (acc_scale = 1 / (wt_scale * x_scale)), so the same GEMM rule holds."""
    with arithmetic(prec):
        base = fc.fwd_case(h, 0)
        x = base["x"] / x_scale
        d = dict(fc.fwd_reference(x, base["w"], base["scale"], base["shift"]), kind="random")
        got = run_fwd(ctx, conv_w(base["w"], base["scale"], base["shift"]), base["level"], x, base["xf"],
                      x_scale=x_scale)
        check_fwd(d, got, prec, f"spec_fwd {h} {prec} x_scale={x_scale}")


@per_level
@per_prec
def test_ffc_spec_inv_fp64(ctx, prec, h):
    """u against irfftn(relu((spec Wfu^T) * scale + shift)) + t1 in float64 (torch.fft.irfftn on the
    non-Hermitian spectrum): the exact set by the transform rule alone, the random set by the propagated
    bound; scale / shift present and absent; t1 non-zero."""
    with arithmetic(prec):
        for i, c in enumerate(fc.INV_CASES):
            if c.get("only", h) != h:
                continue
            d = fc.inv_case(h, i)
            u = run_inv(ctx, conv_w(d["w"], d["scale"], d["shift"]), d["level"], d["spec"], d["t1"])
            ctx.check_range()
            check_inv(d, u, prec, f"spec_inv {h} {prec} {c['name']}")


@per_level
@per_prec
def test_ffc_norm_fp64(ctx, prec, h):
    """out against act(IN([y_l | y_g + u W2^T]) * (1 + gamma) + beta) (+ res) in float64: the exact set by
    the norm rule, the random set by the propagated bound, l and g channels apart; gamma / beta absent, as the
    halves of one [n, 2C] tensor and dense; act none / relu / lrelu; res absent, separate and res == out;
    y == out and separate; dense and wide pitches; eps 1e-5 / 1e-3.  With pad_out: every element of the
    padded plane written, bit-identical to F.pad(out, 1, "reflect"), and out bit-identical to the run
    without it."""
    with arithmetic(prec):
        for i, c in enumerate(fc.NORM_CASES):
            if c.get("only", h) != h:
                continue
            d = fc.norm_case(h, i)
            what = f"norm {h} {prec} {c['name']}"
            cw = conv_w(d["w"], None, None)
            out, pad = run_norm(ctx, cw, d)
            ctx.check_range()
            check_norm(d, out, fc.norm_tol(d, prec), what)
            if pad is not None:
                assert torch.isfinite(pad).all(), f"{what}: pad_out not completely written"
                assert torch.equal(pad, fc.pad_reflect(out)), f"{what}: pad_out is not F.pad(out, 1, 'reflect')"
                out2, _ = run_norm(ctx, cw, d, pad=None)
                assert torch.equal(out, out2), f"{what}: out changes with pad_out"


@per_prec
def test_ffc_norm_refusals(ctx, prec):
    """An activation the kernel does not implement, gamma without beta and a pitch that is no multiple of 4
    are refused (nothing is launched)."""
    with arithmetic(prec):
        d = fc.norm_case(24, 1)                                        # no gamma / beta, act none, in place
        cw = conv_w(d["w"], None, None)
        for name in ("sigmoid", "tanh", "gelu_tanh"):
            with pytest.raises(RuntimeError, match=f"activation {name}"):
                run_norm(ctx, cw, d, act=getattr(ops, "ACT_" + name.upper()))
        with pytest.raises(RuntimeError, match="gamma and beta"):
            run_norm(ctx, cw, d, gamma=torch.zeros(d["n"], d["level"].c, device=DEV), beta=None)
        with pytest.raises(RuntimeError, match="pitch"):
            run_norm(ctx, cw, d, out_extra=2)
        out, _ = run_norm(ctx, cw, d)                                  # and the accepted form still runs
        check_norm(d, out, fc.norm_tol(d, prec), f"norm 24 {prec} after refusals")


# ----------------------------------------------------------------------------- f16x3 range guard
TWO16 = 65536.0          # the power of two beside 6e4: an exact set times it stays exact


def _raises_once(ctx):
    with pytest.raises(ops._lib.S2VError, match="non-finite"):
        ctx.check_range()
    ctx.check_range()                                              # the flag was reset


@pytest.fixture
def f16x3():
    prev = ops.set_precision("f16x3")
    yield "f16x3"
    ops.set_precision(prev)


def test_range_flag_spec_fwd(ctx, f16x3):
    """Calibrated at |x| <= 10, an input 1e6 times larger overflows the f16 operands: the launch sets the
    lane's flag (numerical overflow, never silent); a fresh ConvW calibrated at 6e4 gets a pre-scale and
    stays within the GEMM rule."""
    d = fc.fwd_case(24, 0)
    cw = conv_w(d["w"], d["scale"], d["shift"])
    run_fwd(ctx, cw, d["level"], d["x"] * 10, d["xf"])
    ctx.check_range()
    assert cw._xscale[ops.PREC_F16X3] == 1.0
    run_fwd(ctx, cw, d["level"], d["x"] * 1e6, d["xf"])
    _raises_once(ctx)
    x = d["x"] * 6e4
    cw2 = conv_w(d["w"], d["scale"], d["shift"])
    got = run_fwd(ctx, cw2, d["level"], x, d["xf"])
    ctx.check_range()
    assert cw2._xscale[ops.PREC_F16X3] == ops.x_scale_for(float(x.abs().max())) != 1.0
    check_fwd(dict(fc.fwd_reference(x, d["w"], d["scale"], d["shift"]), kind="random"), got, "f16x3",
              "spec_fwd 24 f16x3 |x| = 6e4")


def test_range_flag_spec_inv(ctx, f16x3):
    """As above for ffc_spec_inv; the pre-scaled run is the exact set times 2^16 with 2^-16 folded into the
    BatchNorm scale: the same G, so u by the transform rule."""
    i = [c["name"] for c in fc.INV_CASES].index("exact-n3-bn")
    d = fc.inv_case(24, i)
    cw = conv_w(d["w"], d["scale"], d["shift"])
    run_inv(ctx, cw, d["level"], d["spec"] * 8, d["t1"])
    ctx.check_range()
    assert cw._xscale[ops.PREC_F16X3] == 1.0
    run_inv(ctx, cw, d["level"], d["spec"] * 1e6, d["t1"])
    _raises_once(ctx)
    cw2 = conv_w(d["w"], d["scale"] / TWO16, d["shift"])
    u = run_inv(ctx, cw2, d["level"], d["spec"] * TWO16, d["t1"])
    ctx.check_range()
    assert cw2._xscale[ops.PREC_F16X3] == ops.x_scale_for(TWO16) != 1.0
    check_inv(d, u, "f16x3", "spec_inv 24 f16x3 |spec| = 2^16")


def test_range_flag_norm(ctx, f16x3):
    """As above for ffc_norm (the st2 GEMM of the g slices); the pre-scaled run is the exact set with u and y
    times 2^16: V stays exact, the normalised output is checked by the norm rule."""
    i = [c["name"] for c in fc.NORM_CASES].index("exact-n3-lrelu")
    d = fc.norm_case(24, i)
    cw = conv_w(d["w"], None, None)
    run_norm(ctx, cw, d, u=d["u"] * 8)
    ctx.check_range()
    assert cw._xscale[ops.PREC_F16X3] == 1.0
    run_norm(ctx, cw, d, u=d["u"] * 1e6)
    _raises_once(ctx)
    y, u = d["yv"] * TWO16, d["u"] * TWO16
    cw2 = conv_w(d["w"], None, None)
    out, _ = run_norm(ctx, cw2, d, y=y, u=u)
    ctx.check_range()
    assert cw2._xscale[ops.PREC_F16X3] == ops.x_scale_for(TWO16) != 1.0
    ref = fc.norm_reference(y, u, d["w"], d["gamma"], d["beta"], d["resv"], fc.ACTS[d["act"]], fc.ALPHA, d["eps"],
                            d["level"].cl)
    v32 = y.clone()
    v32[..., d["level"].cl:] += u @ d["w"].t()
    assert torch.equal(v32.double(), ref["v"])                      # still exact in fp32
    check_norm(dict(d, ref=ref["ref"]), out, fc.NORM_TOL, "norm 24 f16x3 |u| = 2^16")


# ----------------------------------------------------------------------------- the single-pass f16 mode
def test_f16_mode_runs_the_f16x3_kernels():
    """Under set_precision("f16") the three fused kernels are the f16x3 ones (ops.ffc_fused_ok, layout_code):
    bit-identical outputs."""
    fwd, inv, norm = fc.fwd_case(24, 0), fc.inv_case(24, 0), fc.norm_case(24, 0)
    outs = {}
    for mode in ("f16x3", "f16"):
        prev = ops.set_precision(mode)
        try:
            assert ops.ffc_fused_ok()
            ctx = ops.Ctx(DEV)
            t1, spec = run_fwd(ctx, conv_w(fwd["w"], fwd["scale"], fwd["shift"]), fwd["level"], fwd["x"], fwd["xf"])
            u = run_inv(ctx, conv_w(inv["w"], inv["scale"], inv["shift"]), inv["level"], inv["spec"], inv["t1"])
            out, pad = run_norm(ctx, conv_w(norm["w"], None, None), norm)
            ctx.check_range()
            outs[mode] = (t1, spec, u, out, pad)
        finally:
            ops.set_precision(prev)
    for name, a, b in zip(("t1", "spec", "u", "out", "pad"), outs["f16x3"], outs["f16"]):
        assert torch.isfinite(a).all() and torch.equal(a, b), f"f16 mode: {name} differs from f16x3"
