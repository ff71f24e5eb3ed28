"""Inputs, fp64 references and tolerances for the direct tests of LNet's fused FFC kernels (csrc/ffc.hip:
ffc_spec_fwd / ffc_spec_inv / ffc_norm): pure CPU torch, shared by tests/test_ffc_direct_gpu.py (which runs
the kernels) and tests/test_ffc_cases_host.py (which checks that the inputs exercise what they are meant to
and that the references state the model's operation).

The operations, each in float64 from float32-rounded inputs, at the levels (H, C) = (12, 1024), (24, 256),
(48, 128) with cl = C/4, cg = C - cl, cc = cg/2, WF = H/2 + 1, F = H * WF:
  fwd   t1 = relu((x_g W1^T) * scale1 + shift1);  spec = rfftn(t1, (h, w), ortho) as [n, F, 2cc], channel
        part * cc + c (part 0 = re, 1 = im)
  inv   G = relu((spec Wfu^T) * scale_fu + shift_fu) on [n, F, 2cc];
        u = irfftn(complex(G[..., :cc], G[..., cc:]), s=(H, H), ortho) + t1   (torch.fft.irfftn itself: after
        the ReLU the spectrum is not Hermitian-consistent, and what irfftn does with it is the operation)
  norm  V = [y_l | y_g + u W2^T];  out = act((V - mean) / sqrt(var + eps) * (1 + gamma) + beta) (+ res), biased
        variance per (image, channel);  pad = F.pad(out, (1, 1, 1, 1), "reflect")

Operand sets:
  random  x, spec, u, y uniform in [-1, 1), weights uniform in [-1, 1) / sqrt(K), scale in +-[0.5, 1.5] (the
          negative ones make the ReLU cut the other half), shift in [-0.5, 0.5], gamma / beta in (-1, 1), res
          in [-1, 1)
  exact   every GEMM operand, y and shift a multiple of 1/8 with |value| <= 1, scale in {+-1, +-2}: every
          product and partial sum is representable in fp32 and in the bf16 / f16 hi halves with zero lo
          halves, so the GEMM is exact in both arithmetics whatever the summation order, and the stage behind
          it (G -> u, V -> out) is tested at the fp32 tolerance of that stage alone.

Tolerances (none of them new):
  GEMM rule       |err| <= REL[prec] * (B + 1) + 1e-6, REL of tests/test_ops_gpu.py, B = (|A| |W|^T) * |scale|
                  (the ReLU is 1-Lipschitz: the rule holds behind it)
  transform rule  the rule of tests/misc_cases.py: ref32 = the same transform as two separable matrix passes
                  in float32 on the CPU with ops.fft_tables(H, H, "cpu"), e_ref = max|ref32 - ref64|,
                  tol_T = max(4 * e_ref, 16 * 2^-24 * max|ref64|)
  norm rule       the 2e-5 of test_instnorm_adain (unit-variance outputs, gamma in (-1, 1))
  propagated      random sets, where a GEMM error passes through a later stage:
    inv   every coefficient of the ortho irfftn from the half spectrum has modulus <= 2/H, so
          tol_u[n, :, :, c] = (2/H) * sum_f (E_G[n, f, c] + E_G[n, f, cc + c]) + tol_T
    norm  E_V = the GEMM-rule tolerance of u W2^T on the g channels, 0 on the l channels; m = mean_pix E_V,
          M = max_pix E_V, yhat = (V - mean) / sigma: the mean moves by <= m and the std by <= M, so
          tol_out = 1.25 * |1 + gamma| * (E_V + m + |yhat| * M) / sigma + 2e-5 (1.25: the second-order terms;
          condition, checked on the host: sigma >= 0.25 for every (image, channel))
"""
import functools
import math

import torch
import torch.nn.functional as F

import s2v_import  # noqa: F401
from s2v_amd import _lib, ops
from s2v_amd._lib import ACT_LRELU, ACT_NONE, ACT_RELU

EPS24 = 2.0 ** -24
REL = {"f16x3": 3e-6, "bf16x3": 5e-5}          # tests/test_ops_gpu.py REL
NORM_TOL = 2e-5                                # tests/test_ops_gpu.py test_instnorm_adain
LEVELS = (12, 24, 48)
ACTS = {"none": ACT_NONE, "relu": ACT_RELU, "lrelu": ACT_LRELU}
ALPHA = 0.2


class Level:
    """The constants of FfcLevel<H> (csrc/ffc.hip) that the operation itself has."""

    def __init__(self, h):
        self.h = h
        self.c = int(_lib.load().s2v_ffc_channels(h))
        assert self.c > 0, h
        self.cl = self.c // 4
        self.cg = self.c - self.cl
        self.cc = self.cg // 2
        self.wf = h // 2 + 1
        self.f = h * self.wf


@functools.lru_cache(maxsize=None)
def level(h: int) -> Level:
    return Level(h)


# ----------------------------------------------------------------------------- operands
def rand(*shape, seed, lo=-1.0, hi=1.0):
    """Uniform float32 values in [lo, hi) from a seeded generator."""
    g = torch.Generator().manual_seed(seed)
    return (lo + (hi - lo) * torch.rand(*shape, generator=g, dtype=torch.float64)).float()


def eighths(*shape, seed):
    """Multiples of 1/8 in [-1, 1], uniform over the 17 values."""
    g = torch.Generator().manual_seed(seed)
    return (torch.randint(-8, 9, shape, generator=g).double() / 8).float()


def signed(mag: torch.Tensor, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.where(torch.rand(mag.shape, generator=g) < 0.5, -mag, mag)


def operand(kind, *shape, seed):
    return rand(*shape, seed=seed) if kind == "random" else eighths(*shape, seed=seed)


def weight(kind, rows, k, seed):
    return rand(rows, k, seed=seed) / math.sqrt(k) if kind == "random" else eighths(rows, k, seed=seed)


def bn_vectors(kind, ch, seed):
    """(scale, shift) of a folded BatchNorm: random +-[0.5, 1.5] / [-0.5, 0.5]; exact {+-1, +-2} / multiples of
    1/8 in [-0.5, 0.5]."""
    if kind == "random":
        return signed(rand(ch, seed=seed, lo=0.5, hi=1.5), seed + 1), rand(ch, seed=seed + 2, lo=-0.5, hi=0.5)
    g = torch.Generator().manual_seed(seed)
    mag = torch.where(torch.rand(ch, generator=g) < 0.5, 1.0, 2.0)
    return signed(mag, seed + 1), (torch.randint(-4, 5, (ch,), generator=g).double() / 8).float()


def bn_tuple(scale: torch.Tensor, shift: torch.Tensor):
    """A ConvW ``bn=`` tuple (weight, bias, mean, var) with bn_eps = 0 whose fold is exactly (scale, shift):
    s = weight / sqrt(1 + 0) = scale, shift = bias - 0 * s."""
    return scale.clone(), shift.clone(), torch.zeros_like(scale), torch.ones_like(scale)


def gemm_tol(bound: torch.Tensor, prec: str) -> torch.Tensor:
    return REL[prec] * (bound + 1.0) + 1e-6


# ----------------------------------------------------------------------------- transforms
def rfft64(t1: torch.Tensor) -> torch.Tensor:
    """[n, H, W, cc] (any float type) -> the fp64 spectrum [n, F, 2cc], channel part * cc + c."""
    n, h, w, cc = t1.shape
    z = torch.fft.rfftn(t1.double(), dim=(1, 2), norm="ortho")                  # [n, H, WF, cc]
    return torch.cat([z.real, z.imag], -1).reshape(n, h * (w // 2 + 1), 2 * cc)


def irfft64(g: torch.Tensor, h: int) -> torch.Tensor:
    """[n, F, 2cc] -> irfftn(complex(re, im), s=(H, H), ortho) as [n, H, H, cc] in fp64."""
    n, f, c2 = g.shape
    cc, wf = c2 // 2, h // 2 + 1
    z = g.double().reshape(n, h, wf, c2)
    return torch.fft.irfftn(torch.complex(z[..., :cc], z[..., cc:]), s=(h, h), dim=(1, 2), norm="ortho")


def _tables(h):
    wf = h // 2 + 1
    t = ops.fft_tables(h, h, "cpu")
    fw, t = t[:2 * wf * h].reshape(h, 2, wf), t[2 * wf * h:]
    fh, t = t[:2 * h * h].reshape(h, 2, h), t[2 * h * h:]
    ih, t = t[:2 * h * h].reshape(h, 2, h), t[2 * h * h:]
    iw = t.reshape(wf, 2, h)
    return fw, fh, ih, iw


def rfft32(t1: torch.Tensor) -> torch.Tensor:
    """rfft64's transform as a W pass and a complex H pass of float32 matrix products."""
    n, h, w, cc = t1.shape
    fw, fh, _, _ = _tables(h)
    y = torch.einsum("wpv,nhwc->pnhvc", fw, t1.float())
    fr, fi = fh[:, 0], fh[:, 1]
    zr = torch.einsum("hu,nhvc->nuvc", fr, y[0]) - torch.einsum("hu,nhvc->nuvc", fi, y[1])
    zi = torch.einsum("hu,nhvc->nuvc", fr, y[1]) + torch.einsum("hu,nhvc->nuvc", fi, y[0])
    return torch.cat([zr, zi], -1).reshape(n, h * (w // 2 + 1), 2 * cc)


def irfft32(g: torch.Tensor, h: int) -> torch.Tensor:
    """irfft64's transform as a complex inverse H pass and a c2r W pass of float32 matrix products."""
    n, f, c2 = g.shape
    cc, wf = c2 // 2, h // 2 + 1
    _, _, ih, iw = _tables(h)
    z = g.float().reshape(n, h, wf, c2)
    zr, zi = z[..., :cc], z[..., cc:]
    gr, gi = ih[:, 0], ih[:, 1]
    yr = torch.einsum("uh,nuvc->nhvc", gr, zr) - torch.einsum("uh,nuvc->nhvc", gi, zi)
    yi = torch.einsum("uh,nuvc->nhvc", gr, zi) + torch.einsum("uh,nuvc->nhvc", gi, zr)
    return torch.einsum("vw,nhvc->nhwc", iw[:, 0], yr) + torch.einsum("vw,nhvc->nhwc", iw[:, 1], yi)


def transform_tol(ref64: torch.Tensor, ref32: torch.Tensor):
    """(tol_T, e_ref, floor) of the transform rule."""
    e_ref = float((ref32.double() - ref64).abs().max())
    floor = 16 * EPS24 * float(ref64.abs().max())
    return max(4 * e_ref, floor), e_ref, floor


# ----------------------------------------------------------------------------- the case lists
# spec_fwd: xf (the form of x_g): "wide" = channels [cl, cl + cg) of a [n, H, H, C + 8] tensor,
# "dense" = a [n, H, H, cg] tensor.  n = 8 at one level only (``only``).
FWD_CASES = (
    dict(name="rand-n3-wide-bn", kind="random", n=3, xf="wide", bn=True),
    dict(name="rand-n16-dense-nobn", kind="random", n=16, xf="dense", bn=False),
    dict(name="exact-n3-dense-bn", kind="exact", n=3, xf="dense", bn=True),
    dict(name="exact-n16-wide-nobn", kind="exact", n=16, xf="wide", bn=False),
    dict(name="rand-n8-wide-bn", kind="random", n=8, xf="wide", bn=True, only=24),
)
# the explicit x_scale runs of the raw op (on the first FWD case, the input multiplied by 1 / x_scale)
X_SCALES = (2.0 ** -3, 2.0 ** 4)

INV_CASES = (
    dict(name="rand-n3-bn", kind="random", n=3, bn=True),
    dict(name="rand-n16-nobn", kind="random", n=16, bn=False),
    dict(name="exact-n3-bn", kind="exact", n=3, bn=True),
    dict(name="exact-n16-nobn", kind="exact", n=16, bn=False),
    dict(name="rand-n8-bn", kind="random", n=8, bn=True, only=24),
)

# ffc_norm: gb = None | "halves" (gamma / beta the two column halves of one [n, 2C] tensor, row stride 2C) |
# "dense" (two [n, C] tensors); y = "out" (in place) | a pitch; out = a pitch; res = None | "out" (the engine's
# in-place FFC2 form) | a pitch; pad = None | a pitch.  Pitches are C + the number given.
NORM_CASES = (
    dict(name="rand-n3-ffc2", kind="random", n=3, gb="halves", act="lrelu", y=4, out=0, res="out", pad=4, eps=1e-5),
    dict(name="rand-n3-bare", kind="random", n=3, gb=None, act="none", y="out", out=0, res=None, pad=None, eps=1e-3),
    dict(name="rand-n3-relu", kind="random", n=3, gb="dense", act="relu", y="out", out=4, res=4, pad=0, eps=1e-5),
    dict(name="rand-n16-lrelu", kind="random", n=16, gb="halves", act="lrelu", y=0, out=0, res=None, pad=4, eps=1e-5),
    dict(name="exact-n3-lrelu", kind="exact", n=3, gb="halves", act="lrelu", y=4, out=4, res=0, pad=None, eps=1e-5),
    dict(name="exact-n16-relu", kind="exact", n=16, gb=None, act="relu", y="out", out=0, res=None, pad=None, eps=1e-3),
    dict(name="rand-n8-ffc2", kind="random", n=8, gb="halves", act="lrelu", y=4, out=0, res="out", pad=4, eps=1e-5,
         only=24),
)


def cases_of(cases, h):
    return [c for c in cases if c.get("only", h) == h]


def _seed(h, i, k):
    return 100000 * k + 1000 * LEVELS.index(h) + 10 * i


# ----------------------------------------------------------------------------- spec_fwd
@functools.lru_cache(maxsize=6)
def fwd_case(h: int, i: int):
    """Operands and references of FWD_CASES[i] at level h.  x [n, H, H, cg], w [cc, cg], scale / shift [cc] or
    None; t1 [n, H, H, cc] fp64 and its GEMM bound; spec [n, F, 2cc] fp64 of the fp64 t1; (tol_T, e_ref,
    floor) from the float32-rounded reference t1."""
    L, d = level(h), FWD_CASES[i]
    kind, n = d["kind"], d["n"]
    x = operand(kind, n, h, h, L.cg, seed=_seed(h, i, 1))
    w = weight(kind, L.cc, L.cg, _seed(h, i, 2))
    scale, shift = bn_vectors(kind, L.cc, _seed(h, i, 3)) if d["bn"] else (None, None)
    out = dict(d, level=L, x=x, w=w, scale=scale, shift=shift)
    out.update(fwd_reference(x, w, scale, shift))
    return out


def fwd_reference(x, w, scale, shift):
    s = 1.0 if scale is None else scale.double()
    b = 0.0 if shift is None else shift.double()
    t1 = F.relu(x.double() @ w.double().t() * s + b)
    bound = x.double().abs() @ w.double().abs().t() * (1.0 if scale is None else scale.double().abs())
    t32 = t1.float()
    tol_t, e_ref, floor = transform_tol(rfft64(t32), rfft32(t32))
    return dict(t1=t1, bound=bound, spec=rfft64(t1), tol_t=tol_t, e_ref=e_ref, floor=floor)


# ----------------------------------------------------------------------------- spec_inv
@functools.lru_cache(maxsize=6)
def inv_case(h: int, i: int):
    """Operands and references of INV_CASES[i] at level h.  spec [n, F, 2cc], w [2cc, 2cc] in the (part,
    channel) order, scale / shift [2cc] or None, t1 [n, H, H, cc]; G [n, F, 2cc] fp64 with its GEMM bound;
    u [n, H, H, cc] fp64; the transform rule from the float32-rounded G."""
    L, d = level(h), INV_CASES[i]
    kind, n = d["kind"], d["n"]
    spec = operand(kind, n, L.f, 2 * L.cc, seed=_seed(h, i, 4))
    w = weight(kind, 2 * L.cc, 2 * L.cc, _seed(h, i, 5))
    scale, shift = bn_vectors(kind, 2 * L.cc, _seed(h, i, 6)) if d["bn"] else (None, None)
    t1 = operand(kind, n, h, h, L.cc, seed=_seed(h, i, 7))
    out = dict(d, level=L, spec=spec, w=w, scale=scale, shift=shift, t1=t1)
    out.update(inv_reference(spec, w, scale, shift, t1, h))
    return out


def inv_reference(spec, w, scale, shift, t1, h):
    s = 1.0 if scale is None else scale.double()
    b = 0.0 if shift is None else shift.double()
    g = F.relu(spec.double() @ w.double().t() * s + b)
    bound = spec.double().abs() @ w.double().abs().t() * (1.0 if scale is None else scale.double().abs())
    u = irfft64(g, h) + t1.double()
    g32 = g.float()
    tol_t, e_ref, floor = transform_tol(irfft64(g32, h) + t1.double(), irfft32(g32, h) + t1)
    return dict(g=g, bound=bound, u=u, tol_t=tol_t, e_ref=e_ref, floor=floor)


def inv_tol(d, prec: str) -> torch.Tensor:
    """The propagated inv bound [n, 1, 1, cc] of a random case."""
    cc, h = d["level"].cc, d["level"].h
    e_g = gemm_tol(d["bound"], prec)
    return ((2.0 / h) * (e_g[..., :cc] + e_g[..., cc:]).sum(1) + d["tol_t"])[:, None, None, :]


def fourier_unit_model(t1_nchw: torch.Tensor, w_model: torch.Tensor, scale_model: torch.Tensor,
                       shift_model: torch.Tensor):
    """The model's FourierUnit forward in its own channel order, fp64, NCHW: the half spectrum of every
    channel, real and imaginary parts stacked last, moved beside the channel and flattened so that channel c
    becomes the pair (2c, 2c + 1) = (re, im); a 1x1 conv over those 2cc channels, the eval BatchNorm as a
    per-channel scale / shift, ReLU; the pairs taken apart again into a complex half spectrum; irfftn at the
    input size.  Returns (the stacked spectrum [n, 2cc, H, WF], the output [n, cc, H, W])."""
    n, cc, h, w = t1_nchw.shape
    z = torch.fft.rfftn(t1_nchw.double(), dim=(-2, -1), norm="ortho")
    st = torch.stack((z.real, z.imag), dim=-1).permute(0, 1, 4, 2, 3).contiguous().view(n, 2 * cc, h, w // 2 + 1)
    v = torch.einsum("oi,nihw->nohw", w_model.double(), st)
    v = F.relu(v * scale_model.double()[None, :, None, None] + shift_model.double()[None, :, None, None])
    v = v.view(n, cc, 2, h, w // 2 + 1).permute(0, 1, 3, 4, 2).contiguous()
    return st, torch.fft.irfftn(torch.complex(v[..., 0], v[..., 1]), s=(h, w), dim=(-2, -1), norm="ortho")


def fu_perm(cc: int) -> torch.Tensor:
    """engine/lnet.py's reordering of the FourierUnit conv: (part, channel) index i -> model channel."""
    return torch.tensor([2 * (i % cc) + i // cc for i in range(2 * cc)])


# ----------------------------------------------------------------------------- norm
@functools.lru_cache(maxsize=4)
def norm_case(h: int, i: int):
    """Operands and references of NORM_CASES[i] at level h.  y [n, H, H, C], u [n, H, H, cc], w [cg, cc],
    gamma / beta [n, C] or None, res [n, H, H, C] or None; v = [y_l | y_g + u W2^T] fp64 with the bound of
    the product (0 on the l channels), mean / sigma / yhat, out fp64."""
    L, d = level(h), NORM_CASES[i]
    kind, n = d["kind"], d["n"]
    y = operand(kind, n, h, h, L.c, seed=_seed(h, i, 8))
    u = operand(kind, n, h, h, L.cc, seed=_seed(h, i, 9))
    w = weight(kind, L.cg, L.cc, _seed(h, i, 10))
    gamma = beta = res = None
    if d["gb"] is not None:
        gamma = rand(n, L.c, seed=_seed(h, i, 11), lo=-0.999, hi=0.999)
        beta = rand(n, L.c, seed=_seed(h, i, 12), lo=-0.999, hi=0.999)
    if d["res"] is not None:
        res = rand(n, h, h, L.c, seed=_seed(h, i, 13))
    out = dict(d, level=L, yv=y, u=u, w=w, gamma=gamma, beta=beta, resv=res)
    out.update(norm_reference(y, u, w, gamma, beta, res, ACTS[d["act"]], ALPHA, d["eps"], L.cl))
    return out


def norm_reference(y, u, w, gamma, beta, res, act, alpha, eps, cl):
    v = y.double().clone()
    v[..., cl:] += u.double() @ w.double().t()
    bound = torch.zeros_like(v)
    bound[..., cl:] = u.double().abs() @ w.double().abs().t()
    mean = v.mean((1, 2), keepdim=True)
    var = v.var((1, 2), unbiased=False, keepdim=True)
    sigma = torch.sqrt(var + eps)
    yhat = (v - mean) / sigma
    gm = 1.0 if gamma is None else 1.0 + gamma.double()[:, None, None, :]
    bt = 0.0 if beta is None else beta.double()[:, None, None, :]
    o = yhat * gm + bt
    if act == ACT_RELU:
        o = F.relu(o)
    elif act == ACT_LRELU:
        o = F.leaky_relu(o, float(torch.tensor(alpha, dtype=torch.float32)))
    else:
        assert act == ACT_NONE
    if res is not None:
        o = o + res.double()
    return dict(v=v, bound=bound, sigma=sigma, std=torch.sqrt(var), yhat=yhat, gm=gm, ref=o)


def norm_tol(d, prec: str) -> torch.Tensor:
    """The per-element tolerance of a norm case: the norm rule for the exact set (V is exact), the
    propagated bound for the random set."""
    if d["kind"] == "exact":
        return torch.full_like(d["ref"], NORM_TOL)
    cl = d["level"].cl
    e_v = torch.zeros_like(d["v"])
    e_v[..., cl:] = gemm_tol(d["bound"][..., cl:], prec)
    m = e_v.mean((1, 2), keepdim=True)
    big = e_v.amax((1, 2), keepdim=True)
    gm = d["gm"] if torch.is_tensor(d["gm"]) else torch.tensor(d["gm"], dtype=torch.float64)
    return 1.25 * gm.abs() * (e_v + m + d["yhat"].abs() * big) / d["sigma"] + NORM_TOL


def pad_reflect(out_nhwc: torch.Tensor) -> torch.Tensor:
    """F.pad(out, (1, 1, 1, 1), "reflect") of an NHWC tensor."""
    return F.pad(out_nhwc.permute(0, 3, 1, 2), (1, 1, 1, 1), mode="reflect").permute(0, 2, 3, 1).contiguous()
