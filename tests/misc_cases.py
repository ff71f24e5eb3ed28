"""Inputs and fp64 references for the direct tests of the small non-conv kernels (flow warp, attention,
token LayerNorm, eltwise, amax): pure CPU torch / numpy, shared by tests/test_misc_ops_gpu.py (which
runs the kernels) and tests/test_misc_cases_host.py (which checks that the inputs exercise what they
are meant to).

Tolerance rule (flow warp, attention, LayerNorm): every case carries ``ref64`` (the formula in
float64), ``ref32`` (the same formula in float32 on the CPU) and ``e_ref = max|ref32 - ref64|``; a
kernel passes when ``max|got - ref64| <= max(4 * e_ref, floor)`` with ``floor = 16 * 2^-24 *
max|ref64|`` for the cases whose fp32 reference happens to be exact.  The factor 4 allows another
legitimate fp32 operation order (fma contraction, reciprocal instead of division, the reduction
tree); a wrong tap, index, weight or branch on data in [-1, 1] is four orders of magnitude above it.
"""
import functools
import math

import torch
import torch.nn.functional as F

import s2v_import  # noqa: F401
from s2v_amd._lib import ACT_GELU_TANH, ACT_LRELU, ACT_NONE, ACT_RELU, ACT_SIGMOID, ACT_TANH

EPS24 = 2.0 ** -24
EPS23 = 2.0 ** -23


def rand(*shape, seed, lo=-1.0, hi=1.0):
    """Uniform float32 values in [lo, hi) from a seeded generator."""
    g = torch.Generator().manual_seed(seed)
    return (lo + (hi - lo) * torch.rand(*shape, generator=g, dtype=torch.float64)).float()


def tolerance(ref64: torch.Tensor, ref32: torch.Tensor):
    """(tol, e_ref, floor) of the common tolerance rule."""
    e_ref = float((ref32.double() - ref64).abs().max())
    floor = 16 * EPS24 * float(ref64.abs().max())
    return max(4 * e_ref, floor), e_ref, floor


# ----------------------------------------------------------------------------- flow warp
# (name, n, c, h, w, fh, fw, flow amplitude in flow pixels, source form, flow form, output form)
#   source: "nchw" contiguous, "nhwc" a permuted NHWC tensor (channel stride 1), "slice" channels
#           [1, 1 + c) of a wider NCHW tensor
#   flow:   "dense" 2-channel NHWC, "slice" channels [1, 3) of a 4-channel NHWC tensor
#   output: "dense", "slice" channels [3, 3 + c) of a wider NaN-filled NHWC tensor
WARP_CASES = (
    ("16blk", 2, 5, 37, 53, 10, 14, 4.0, "nhwc", "slice", "slice"),
    ("same", 3, 3, 33, 29, 33, 29, 12.0, "slice", "dense", "dense"),
    ("12full", 1, 4, 64, 48, 16, 12, 3.0, "nchw", "slice", "slice"),
    ("1axis", 1, 3, 50, 47, 25, 47, 2.0, "nhwc", "dense", "dense"),
    ("tiny", 1, 2, 9, 11, 2, 2, 1.0, "slice", "slice", "slice"),
    ("patch", 2, 3, 40, 36, 40, 36, 3.0, "nchw", "dense", "slice"),
)
# the "patch" case: flow rows / columns [PATCH) of every image are +-1e4 flow pixels (far outside)
PATCH = (slice(8, 20), slice(5, 17))
PATCH_FLOW = 1.0e4
BAND = slice(26, 34)


def warp_blocks(case):
    _, n, _, h, w = case[:5]
    return -(-(n * h * w) // 256)


@functools.lru_cache(maxsize=None)
def warp_case(i: int):
    """Inputs (float32, NCHW) and references of WARP_CASES[i]."""
    from oracle import nets
    name, n, c, h, w, fh, fw, amp = WARP_CASES[i][:8]
    flow = rand(n, 2, fh, fw, seed=100 + i, lo=-amp, hi=amp)
    src = rand(n, c, h, w, seed=200 + i)
    patch = None
    if name == "patch":
        sign = torch.where(rand(n, 2, fh, fw, seed=300 + i) < 0, -1.0, 1.0)
        patch = torch.zeros(n, 1, h, w, dtype=torch.bool)
        patch[:, :, PATCH[0], PATCH[1]] = True
        flow = torch.where(patch, sign * PATCH_FLOW, flow)
        # rows [BAND): x flow -ox + U[-0.3, 0.3] puts every sample between columns -1 and 0, where the
        # two left taps are outside the image and the two right ones inside
        to_band = rand(n, fh, fw, seed=350 + i, lo=-0.3, hi=0.3) - torch.arange(fw, dtype=torch.float32)
        flow[:, 0, BAND] = to_band[:, BAND]
    ref64 = nets.warp_image(src.double(), nets.flow_to_deformation(flow.double()))
    ref32 = nets.warp_image(src, nets.flow_to_deformation(flow))
    tol, e_ref, floor = tolerance(ref64, ref32)
    return dict(name=name, flow=flow, src=src, ref64=ref64, ref32=ref32, tol=tol, e_ref=e_ref, floor=floor,
                patch=patch)


def warp_sample_coords(flow: torch.Tensor, h: int, w: int):
    """fp64 source pixel coordinates (ix, iy), each [n, h, w], that grid_sample (align_corners=False)
    reads for the flow of a warp case."""
    from oracle import nets
    d = nets.flow_to_deformation(flow.double())
    if tuple(d.shape[1:3]) != (h, w):
        d = F.interpolate(d.permute(0, 3, 1, 2), size=(h, w), mode="bilinear", align_corners=False).permute(0, 2, 3, 1)
    return ((d[..., 0] + 1) * w - 1) / 2, ((d[..., 1] + 1) * h - 1) / 2


def warp_taps_outside(flow: torch.Tensor, h: int, w: int) -> torch.Tensor:
    """Number of the four bilinear taps (0 .. 4) that fall outside the image, per output pixel."""
    ix, iy = warp_sample_coords(flow, h, w)
    x0, y0 = torch.floor(ix), torch.floor(iy)
    out = torch.zeros_like(ix, dtype=torch.int64)
    for dy in (0, 1):
        for dx in (0, 1):
            xx, yy = x0 + dx, y0 + dy
            out += ((xx < 0) | (xx > w - 1) | (yy < 0) | (yy > h - 1)).long()
    return out


# ----------------------------------------------------------------------------- attention
# (batch, tokens, heads, magnitude of q and k); v is in [-1, 1]; dim_head 64, scale 1/8
ATTN_CASES = (
    (1, 256, 2, 1.0),
    (3, 1, 1, 1.0),
    (2, 3, 2, 1.0),
    (2, 65, 3, 6.0),
    (1, 200, 1, 12.0),
    (64, 5, 8, 1.0),
    (2, 12, 1, 1.0),
)


def _attention(q, k, v, b, T, heads):
    def split(t):
        return t.reshape(b, T, heads, 64).transpose(1, 2)
    logits = split(q) @ split(k).transpose(-1, -2) * 0.125
    return (torch.softmax(logits, -1) @ split(v)).transpose(1, 2).reshape(b * T, heads * 64), logits


@functools.lru_cache(maxsize=None)
def attn_case(i: int):
    """q, k, v as [batch * tokens, heads * 64] float32 rows, and the references."""
    b, T, heads, mag = ATTN_CASES[i]
    hc = heads * 64
    q = rand(b * T, hc, seed=400 + i, lo=-mag, hi=mag)
    k = rand(b * T, hc, seed=420 + i, lo=-mag, hi=mag)
    v = rand(b * T, hc, seed=440 + i)
    ref64, logits = _attention(q.double(), k.double(), v.double(), b, T, heads)
    ref32, _ = _attention(q, k, v, b, T, heads)
    tol, e_ref, floor = tolerance(ref64, ref32)
    return dict(q=q, k=k, v=v, ref64=ref64, ref32=ref32, tol=tol, e_ref=e_ref, floor=floor,
                max_logit=float(logits.abs().max()))


# ----------------------------------------------------------------------------- token LayerNorm
# (rows, dim, mean offset, spread): x = offset + spread * U[-1, 1]
LN_CASES = (
    (5, 512, 1000.0, 1.0),
    (7, 100, 0.0, 1.0),
    (3, 1, 0.0, 1.0),
    (9, 63, 50.0, 0.01),
    (4, 65, 0.0, 1.0),
    (288, 512, 0.0, 1.0),
)
LN_EPS = 1e-5


@functools.lru_cache(maxsize=None)
def ln_case(i: int):
    rows, dim, off, spread = LN_CASES[i]
    x = (off + spread * rand(rows, dim, seed=500 + i).double()).float()
    w, b = rand(dim, seed=520 + i), rand(dim, seed=540 + i)
    ref64 = F.layer_norm(x.double(), (dim,), w.double(), b.double(), LN_EPS)
    ref32 = F.layer_norm(x, (dim,), w, b, LN_EPS)
    tol, e_ref, floor = tolerance(ref64, ref32)
    return dict(x=x, w=w, b=b, ref64=ref64, ref32=ref32, tol=tol, e_ref=e_ref, floor=floor)


# ----------------------------------------------------------------------------- eltwise
ACTS = {"none": ACT_NONE, "relu": ACT_RELU, "lrelu": ACT_LRELU, "sigmoid": ACT_SIGMOID, "tanh": ACT_TANH,
        "gelu_tanh": ACT_GELU_TANH}
ELT_NHW = (3, 7, 5)            # 105 pixels: no multiple of 64

# A view is (pitch, channel offset) of a [3, 7, 5, pitch] tensor.  Layout "a" (c = 8, every pitch a
# multiple of 4, every offset 16-byte aligned) is the float4 kernel; "b" (c = 6) the scalar one.
_LAYOUT = {"a": dict(c=8, x=(12, 4), y=(16, 8), mul=(8, 0), add=(12, 4)),
           "b": dict(c=6, x=(9, 2), y=(7, 1), mul=(6, 0), add=(8, 1))}


def _elt(name, layout, *, mul=True, add=True, bias="own", a=1.0, act="none", alpha=0.0, post=1.0, **over):
    """One eltwise case.  bias: None, "own" (a tensor of c values) or "offset" (b[1:1 + c] of a longer
    one).  y: a (pitch, offset) view, or "x" for in place.  add: a view, or "y" for the output view."""
    d = dict(_LAYOUT[layout])
    if mul is not True:
        d["mul"] = mul or None
    if add is not True:
        d["add"] = add or None
    d.update(name=name, bias=bias, a=a, act=act, alpha=alpha, post=post)
    d.update(over)
    return d


def _elt_cases():
    cases = []
    for lay in "ab":
        for m in (False, True):
            for ad in (False, True):
                for bi in (None, "own"):
                    cases.append(_elt(f"{lay}-mul{int(m)}-add{int(ad)}-bias{int(bi is not None)}", lay, mul=m, add=ad,
                                      bias=bi, a=0.5))
    # c = 8 layouts that must take the scalar kernel
    cases.append(_elt("x-offset2-of-12", "a", x=(12, 2)))
    cases.append(_elt("mul-pitch10", "a", mul=(10, 0)))
    cases.append(_elt("bias-offset1", "a", bias="offset"))
    for lay in "ab":
        for act in ACTS:
            cases.append(_elt(f"{lay}-{act}", lay, act=act, alpha=0.2, post=math.sqrt(2.0)))
    # GFPGAN SFT: in place on a channel slice, y = x * scale + shift
    cases.append(_elt("sft-aligned", "a", x=(16, 4), y="x", bias=None))
    cases.append(_elt("sft-unaligned", "a", x=(16, 3), y="x", bias=None))
    # RRDB residual: y = 0.2 * x + y
    cases.append(_elt("rrdb-aligned", "a", mul=False, add="y", bias=None, a=0.2))
    cases.append(_elt("rrdb-scalar", "b", mul=False, add="y", bias=None, a=0.2))
    return tuple(cases)


ELT_CASES = _elt_cases()


def act_ref(v, act, alpha):
    if act == ACT_RELU:
        return F.relu(v)
    if act == ACT_LRELU:
        return F.leaky_relu(v, alpha)
    if act == ACT_SIGMOID:
        return torch.sigmoid(v)
    if act == ACT_TANH:
        return torch.tanh(v)
    if act == ACT_GELU_TANH:
        return 0.5 * v * (1 + torch.tanh(math.sqrt(2 / math.pi) * (v + 0.044715 * v ** 3)))
    return v


def f32(s: float) -> float:
    """The float32 value the kernel receives for a scalar argument."""
    return float(torch.tensor(s, dtype=torch.float32))


@functools.lru_cache(maxsize=None)
def elt_case(i: int):
    """Values (float32 [3, 7, 5, c] / [c]), the fp64 reference ``post * act(x * a * mul + add + bias)``,
    the per-element bound and the CPU fp32 evaluation.  The scalars a / alpha / post enter the
    reference as the float32 values the C ABI passes; x * a * mul + add + bias ranges over about
    [-6, 6], so the sigmoid / tanh tails and the knee of the GELU are sampled."""
    d = ELT_CASES[i]
    c, shape = d["c"], ELT_NHW + (d["c"],)
    a, alpha, post, act = f32(d["a"]), f32(d["alpha"]), f32(d["post"]), ACTS[d["act"]]
    x = rand(*shape, seed=600 + i, lo=-2.0, hi=2.0)
    mul = rand(*shape, seed=700 + i, lo=-1.5, hi=1.5) if d["mul"] is not None else None
    add = rand(*shape, seed=800 + i, lo=-2.0, hi=2.0) if d["add"] is not None else None
    bias = rand(c + 4, seed=900 + i)[1:1 + c].clone() if d["bias"] is not None else None

    def formula(dt):
        v = x.to(dt) * torch.tensor(a, dtype=dt)
        if mul is not None:
            v = v * mul.to(dt)
        prod = v.abs()
        if add is not None:
            v = v + add.to(dt)
        if bias is not None:
            v = v + bias.to(dt)
        return act_ref(v, act, alpha) * torch.tensor(post, dtype=dt), prod
    ref64, prod = formula(torch.float64)
    ref32, _ = formula(torch.float32)
    mag = prod + (add.double().abs() if add is not None else 0) + (bias.double().abs() if bias is not None else 0)
    if d["act"] in ("none", "relu", "lrelu"):
        bound = 4 * EPS23 * mag * abs(post) + 1e-30
    else:
        bound = 8 * EPS23 * (mag + 1) * abs(post)
    return dict(spec=d, x=x, mul=mul, add=add, bias=bias, a=a, alpha=alpha, post=post, act=act, ref64=ref64,
                ref32=ref32, bound=bound)


# ----------------------------------------------------------------------------- amax
# (name, (n, h, w), c, pitch, channel offset).  Channels outside the view hold 1e6 and must be ignored.
AMAX_CASES = (
    ("c4-dense", (2, 5, 7), 4, 4, 0),               # float4 rows, one quad per row, one lane per row
    ("c12-pitch16", (1, 9, 11), 12, 16, 0),         # three quads on four lanes, the fourth idle
    ("c256-8197px", (1, 7, 1171), 256, 256, 0),     # 64 lanes per row, grid-stride past 2048 blocks x 4 rows
    ("c130-pitch131", (1, 3, 5), 130, 131, 0),      # scalar: two strides of 64 lanes plus a tail
    ("c1-524289px", (1, 3, 174763), 1, 1, 0),       # scalar, one lane per row, past 2048 x 256 rows
    ("c8-offset2", (2, 4, 6), 8, 12, 2),            # misaligned: scalar, neighbours on both sides
)
AMAX_NEIGHBOUR = 1.0e6
AMAX_PEAK = 3.5
# where the maximum goes: (name, sign); positions are resolved by amax_position
AMAX_PLACEMENTS = (("first", 1.0), ("last", 1.0), ("mid-lastch", 1.0), ("last-negative", -1.0))


def amax_position(place: str, pixels: int, c: int):
    """(pixel, channel) of a placement."""
    if place == "first":
        return 0, 0
    if place.startswith("last"):
        return pixels - 1, c - 1
    return pixels // 2, c - 1


@functools.lru_cache(maxsize=None)
def amax_base(i: int) -> torch.Tensor:
    """The full [n, h, w, pitch] float32 tensor of AMAX_CASES[i]: U[-1, 1] in the view, 1e6 beside it."""
    _, nhw, c, pitch, off = AMAX_CASES[i]
    t = torch.full(nhw + (pitch,), AMAX_NEIGHBOUR)
    t[..., off:off + c] = rand(*nhw, c, seed=1000 + i)
    return t
