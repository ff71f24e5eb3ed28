"""Inputs, fp64 references and bounds for the direct tests of the normalisation kernels of csrc/norm.hip
(LayerNorm2d, InstanceNorm / ADAIN with its reflect-padded second output) and the data-movement kernels of
csrc/misc.hip (resize, pad_reflect, row_pack): pure CPU torch, shared by tests/test_norm_direct_gpu.py (which
runs the kernels) and tests/test_norm_cases_host.py (which checks that the tables reach what they claim and
that the bounds can tell a wrong kernel from a right one).

Bound of the two norms, per element, from the reference's own fp64 ``mean`` and ``rstd``:

    bound = K * 2^-24 * ((|x| + |mean|) * rstd * |scale| + |shift| + |res|) + 2^-126

with (scale, shift) = (weight, bias) for LayerNorm2d and (1 + gamma, beta) for InstanceNorm; a pooled output
takes the mean of its four pixels' bounds.  K is the smallest power of two for which two plain CPU float32
evaluations stay within half the bound on every element of every case: the torch form ``(x - mean) * rstd * g
+ b`` and the kernel's ``fma(x, rstd * g, b - mean * rstd * g)`` (the fma as a float64 product and sum rounded
once to float32), both with mean and var taken from fp64 and rounded to float32.

    K = 16.  Worst err / bound with K = 16: torch form 0.273 (LayerNorm2d ``cap64``, not pooled; 0.265 at
    InstanceNorm ``c260-70x40``), fma form 0.255 (InstanceNorm ``c260-33x31``); with K = 8 the torch form
    reaches 0.546, above one half.  (tests/test_norm_cases_host.py recomputes both and fails if K is no
    longer the smallest.  The third digit moves with the host: the order of the float64 reductions decides
    how a variance rounds to float32.)

Resize follows the tolerance rule of tests/misc_cases.py, ``max(4 * e_ref, 16 * 2^-24 * max|ref64|)``, with
the source coordinate and the two weights computed in float32 as torch's area_pixel_compute_source_index
does and the four taps combined in float64; nearest resize, pad_reflect and row_pack are bit-exact.
"""
import functools

import torch
import torch.nn.functional as F

import misc_cases as mc
from misc_cases import EPS24, act_ref, f32, rand, tolerance  # noqa: F401
from s2v_amd._lib import ACT_LRELU, ACT_NONE, ACT_RELU

K_BOUND = 16
TINY = 2.0 ** -126


def aligned(view) -> bool:
    """A (pitch, offset) channel view of a 16-byte aligned tensor whose float4 accesses stay aligned."""
    return view is None or (view[0] % 4 == 0 and view[1] % 4 == 0)


def fma32(a: torch.Tensor, b: torch.Tensor, c: torch.Tensor) -> torch.Tensor:
    """float32 fma(a, b, c): the float64 product of two float32 values is exact, the sum rounds to 53 bits
    and then to 24."""
    return (a.double() * b.double() + c.double()).float()


def _norm_eval(x, mean, var, eps, scale, shift, act, alpha, pool, res):
    """The fp64 reference, its bound (K_BOUND = 1 units: the caller multiplies) and the two float32
    evaluations of act((x - mean) * rstd * scale + shift) [-> 2x2 mean] + res.  x [n, h, w, c] float32;
    mean / var fp64 broadcastable to x; scale / shift float32 broadcastable to x; res float32 or None."""
    def pooled(t):
        if not pool:
            return t
        n, h, w, c = t.shape
        t = t[:, :h // 2 * 2, :w // 2 * 2]
        return (t[:, 0::2, 0::2] + t[:, 0::2, 1::2] + t[:, 1::2, 0::2] + t[:, 1::2, 1::2]) * 0.25

    x64, s64, b64 = x.double(), scale.double(), shift.double()
    rstd = 1.0 / torch.sqrt(var + eps)
    ref64 = pooled(act_ref((x64 - mean) * rstd * s64 + b64, act, alpha))
    unit = pooled(((x64.abs() + mean.abs()) * rstd * s64.abs() + b64.abs()).expand_as(x64))
    m32, v32, e32 = mean.float(), var.float(), torch.tensor(eps, dtype=torch.float32)
    r32 = 1.0 / torch.sqrt(v32 + e32)
    a32 = alpha                                  # a float32 value already (misc_cases.f32)
    t32 = pooled(act_ref((x - m32) * r32 * scale + shift, act, a32))
    g32 = r32 * scale
    k32 = pooled(act_ref(fma32(x, g32.expand_as(x), (shift - m32 * r32 * scale).expand_as(x)), act, a32))
    if res is not None:
        ref64, unit = ref64 + res.double(), unit + res.double().abs()
        t32, k32 = t32 + res, k32 + res
    return dict(ref64=ref64, unit=EPS24 * unit, mean=mean, rstd=rstd, torch32=t32, fma32=k32)


def bound_of(d) -> torch.Tensor:
    return K_BOUND * d["unit"] + TINY


# ----------------------------------------------------------------------------- LayerNorm2d
# A view is (pitch, channel offset) of an [n, h, w, pitch] tensor; res None = no residual.  values: "unit"
# U[-2, 1.5), "offset" 30 + U[-0.5, 0.5), "const" 0.75 everywhere.
def _ln(name, n, h, w, c, *, x=None, y=None, res=None, act=ACT_NONE, alpha=0.0, eps=1e-5, pools=(False, True),
        values="unit", stats, apply):
    dense = (c, 0)
    return dict(name=name, n=n, h=h, w=w, c=c, x=x or dense, y=y or dense, res=res, act=act, alpha=alpha, eps=eps,
                pools=pools, values=values, stats=stats, apply=apply)


LN_CASES = (
    # four loads in flight in the statistics, 33 statistics blocks per image, apply grid capped at 64 blocks
    # of the 66 the quads need: blocks 0 and 1 take a second LN_EPT step, the other 62 do not
    _ln("cap64", 16, 66, 64, 64, act=ACT_LRELU, alpha=0.1, stats="dense4", apply="vec"),
    # the same cap with 16 quads over 66 full steps: the second step of block 2 breaks after its first quad
    # group; 65 x 65 pools to 32 x 32
    _ln("cap64-odd", 16, 65, 65, 64, act=ACT_RELU, stats="dense4", apply="vec"),
    _ln("odd-slice", 3, 7, 5, 8, x=(16, 4), y=(16, 4), res=(16, 4), act=ACT_RELU, eps=1e-3, stats="strided4",
        apply="vec"),
    _ln("scalar", 2, 9, 7, 6, y=(7, 1), res=(6, 0), stats="scalar", apply="scalar"),
    _ln("misaligned", 2, 6, 6, 8, x=(12, 2), y=(12, 2), res=(12, 2), act=ACT_LRELU, alpha=0.2, eps=1e-3,
        stats="scalar", apply="scalar"),
    _ln("empty-blocks", 2, 3, 1, 16384, pools=(False,), stats="dense4", apply="vec"),
    _ln("offset", 2, 8, 8, 32, act=ACT_LRELU, alpha=0.1, values="offset", stats="dense4", apply="vec"),
    _ln("const", 2, 4, 6, 8, res=(8, 0), act=ACT_RELU, values="const", stats="dense4", apply="vec"),
    # 60 reduced elements: where the unbiased / biased variance differ by 1 / 120; one quad per pixel
    _ln("small", 3, 5, 3, 4, res=(4, 0), act=ACT_LRELU, alpha=0.1, eps=1e-3, stats="dense4", apply="vec"),
)
LN_IDS = [f"{c['name']}-pool{int(p)}" for c in LN_CASES for p in c["pools"]]
LN_RUNS = [(i, p) for i, c in enumerate(LN_CASES) for p in c["pools"]]


def _values(kind, shape, seed):
    if kind == "offset":
        return (30.0 + rand(*shape, seed=seed, lo=-0.5, hi=0.5).double()).float()
    if kind == "const":
        return torch.full(shape, 0.75)
    return rand(*shape, seed=seed, lo=-2.0, hi=1.5)


@functools.lru_cache(maxsize=None)
def ln_inputs(i: int):
    s = LN_CASES[i]
    n, h, w, c = s["n"], s["h"], s["w"], s["c"]
    return dict(x=_values(s["values"], (n, h, w, c), 2000 + i), weight=rand(c, seed=2100 + i),
                bias=rand(c, seed=2200 + i))


def ln_moments(x: torch.Tensor):
    """fp64 mean and biased variance over (H, W, C) of an [n, h, w, c] float32 tensor."""
    x64 = x.double()
    mean = x64.mean(dim=(1, 2, 3), keepdim=True)
    return mean, ((x64 - mean) ** 2).mean(dim=(1, 2, 3), keepdim=True)


@functools.lru_cache(maxsize=None)
def ln_case(i: int, pool: bool):
    """LN_CASES[i] with the given pool setting: inputs [n, h, w, c] float32, the residual at the output size,
    ref64, the per-element bound and the two float32 evaluations."""
    s, d = LN_CASES[i], dict(ln_inputs(i))
    n, h, w, c = s["n"], s["h"], s["w"], s["c"]
    oh, ow = (h // 2, w // 2) if pool else (h, w)
    d["res"] = rand(n, oh, ow, c, seed=2300 + 2 * i + pool) if s["res"] is not None else None
    mean, var = ln_moments(d["x"])
    d.update(_norm_eval(d["x"], mean, var, f32(s["eps"]), d["weight"], d["bias"], s["act"], f32(s["alpha"]), pool,
                        d["res"]))
    d["spec"] = s
    return d


# ----------------------------------------------------------------------------- InstanceNorm / ADAIN
IN_PLANES = ((1, 1), (2, 2), (2, 7), (3, 3), (3, 5), (5, 3), (33, 31), (70, 40))
IN_ACTS = ((ACT_NONE, 0.0), (ACT_RELU, 0.0), (ACT_LRELU, 0.01))
IN_FUSED_MAX = 1023


def _in_cases():
    cases = []

    def add(c, h, w, *, path, x=None, y=None, pad=None, values="unit"):
        i = len(cases)
        act, alpha = IN_ACTS[i % 3]
        vec = path == "vector"
        cases.append(dict(
            name=f"c{c}-{h}x{w}" + ("" if values == "unit" else "-" + values) + ("" if x is None else f"-x{x[0]}.{x[1]}"),
            n=(1, 3)[i % 2], h=h, w=w, c=c, path=path, values=values,
            x=x or ((c, 0) if i % 4 < 2 else (c + 4, 4) if vec else (c + 3, 1)),
            y=y or ((c + 4, 0) if vec else (c + 1, 1)),
            # gamma / beta: None, or columns [0, c) and [c + 4, 2 c + 4) of one [n, 2 c + 4] tensor
            gb=(i // 2) % 3 != 2,
            res=(None, (c + 8, 4) if vec else (c + 2, 1))[(i // 3) % 2],
            act=act, alpha=alpha, eps=(1e-5, 1e-3)[(i // 2) % 2],
            # the reflect-padded second output: channels [4, 4 + c) of a NaN-filled tensor of pitch c + 8
            pad=(c + 8, 4) if vec and h >= 2 and w >= 2 else None))

    for c in (4, 40, 260):
        for h, w in IN_PLANES:
            add(c, h, w, path="vector")
    for h, w in ((1, 1), (3, 5), (33, 31)):
        add(6, h, w, path="scalar")
    for h, w in ((2, 7), (5, 3)):
        add(8, h, w, path="scalar", x=(12, 2), y=(12, 2))
    add(32, 12, 12, path="vector", values="offset")
    return tuple(cases)


IN_CASES = _in_cases()


def in_forms(s):
    """The launch forms a case runs in: "fused" (one launch, TUNE_IN_FUSED = h * w) and "two" (statistics and
    apply launches, TUNE_IN_FUSED = 0) for vector cases of at most 1023 pixels, else the two launches alone
    (the scalar kernels have no fused form)."""
    return ("fused", "two") if s["path"] == "vector" and s["h"] * s["w"] <= IN_FUSED_MAX else ("two",)


IN_RUNS = [(i, f) for i, s in enumerate(IN_CASES) for f in in_forms(s)]
IN_IDS = [f"{IN_CASES[i]['name']}-{f}" for i, f in IN_RUNS]


@functools.lru_cache(maxsize=None)
def in_case(i: int):
    s = IN_CASES[i]
    n, h, w, c = s["n"], s["h"], s["w"], s["c"]
    x = _values(s["values"], (n, h, w, c), 3000 + i)
    gb = rand(n, 2 * c + 4, seed=3100 + i) if s["gb"] else None
    gamma, beta = (gb[:, :c], gb[:, c + 4:]) if s["gb"] else (None, None)
    res = rand(n, h, w, c, seed=3200 + i) if s["res"] is not None else None
    x64 = x.double()
    mean = x64.mean(dim=(1, 2), keepdim=True)
    var = ((x64 - mean) ** 2).mean(dim=(1, 2), keepdim=True)
    scale = 1.0 + gamma[:, None, None, :] if s["gb"] else torch.ones(1, 1, 1, c)
    shift = beta[:, None, None, :] if s["gb"] else torch.zeros(1, 1, 1, c)
    d = _norm_eval(x, mean, var, f32(s["eps"]), scale, shift, s["act"], f32(s["alpha"]), False, res)
    d.update(spec=s, x=x, gb=gb, res=res)
    return d


# ----------------------------------------------------------------------------- resize
def bilinear_taps(scale: float, in_size: int, out_size: int):
    """(i0, i1, l0, l1) of every output index, in float32 as torch's area_pixel_compute_source_index
    (align_corners=False) and the kernels' bilin_index compute them, and the unclamped coordinate.
    ``scale * (dst + 0.5) - 0.5`` is rounded once, as the contracted multiply-subtract of the CPU build of
    F.interpolate rounds it (two roundings move the coordinate by an ulp on some outputs and the result
    by up to 3.6e-6 against F.interpolate; rounded once the two agree to 1.3e-7 on every case)."""
    dst = torch.arange(out_size, dtype=torch.float32)
    raw = (torch.tensor(scale, dtype=torch.float32).double() * (dst + 0.5).double() - 0.5).float()
    src = raw.clamp(min=0.0)
    i0 = src.to(torch.int64)
    i1 = i0 + (i0 < in_size - 1).long()
    l1 = src - i0.float()
    return i0, i1, 1.0 - l1, l1, raw


def bilinear_ref64(x: torch.Tensor, oh: int, ow: int, sh: float, sw: float, shift=0, coords=bilinear_taps):
    """x [n, c, ih, iw] float32 -> fp64 [n, c, oh, ow]: float32 indices and weights, taps combined in
    float64.  ``shift`` moves the second tap by that many pixels (the host test's wrong variant)."""
    ih, iw = x.shape[2:]
    y0, y1, ly0, ly1 = coords(sh, ih, oh)[:4]
    x0, x1, lx0, lx1 = coords(sw, iw, ow)[:4]
    y1, x1 = (y1 + shift).clamp(max=ih - 1), (x1 + shift).clamp(max=iw - 1)
    x64 = x.double()
    ly0, ly1 = ly0.double()[:, None], ly1.double()[:, None]
    lx0, lx1 = lx0.double(), lx1.double()
    top = lx0 * x64[:, :, y0][:, :, :, x0] + lx1 * x64[:, :, y0][:, :, :, x1]
    bot = lx0 * x64[:, :, y1][:, :, :, x0] + lx1 * x64[:, :, y1][:, :, :, x1]
    return ly0 * top + ly1 * bot


def nearest_index(scale: float, in_size: int, out_size: int) -> torch.Tensor:
    """min(floor(dst * scale), in - 1) in float32: torch's nearest_neighbor_compute_source_index."""
    dst = torch.arange(out_size, dtype=torch.float32)
    return torch.floor(dst * torch.tensor(scale, dtype=torch.float32)).long().clamp(max=in_size - 1)


# (name, kernel, n, c, ih, iw, size, scale_factor, modes); the layouts live in the GPU test by name.
#   kernel "generic": resize_kernel; "float4": resize_nhwc4_kernel; "x2": up2_bilinear_nhwc4_kernel with
#   TUNE_RESIZE_UP2 = 1 and resize_nhwc4_kernel with 0 (bilinear), resize_nhwc4_kernel (nearest)
RESIZE_CASES = (
    ("nchw-to-nhwc", "generic", 2, 3, 37, 29, (53, 41), None, (0, 1)),
    ("nhwc-crop-to-nchw", "generic", 2, 5, 7, 6, (7, 6), None, (0, 1)),       # the (2, 3) window of a 12 x 10 image
    ("flip-c3", "generic", 2, 3, 21, 17, (30, 23), None, (0, 1)),             # x stride -3, offset at the row end
    ("slices-by-size", "float4", 2, 8, 100, 90, (37, 53), None, (0, 1)),      # channels [4, 12) of pitch 16, both sides
    ("half", "float4", 2, 8, 40, 36, None, 0.5, (0, 1)),
    ("batch-stride", "float4", 2, 8, 10, 12, (15, 9), None, (0, 1)),          # images 0 and 2 of a batch of 4
    ("flip-c8", "float4", 1, 8, 9, 11, (13, 16), None, (0, 1)),               # x stride -8, offset at the row end
    ("x3", "float4", 1, 8, 20, 20, None, 3, (0, 1)),
    ("1x1-up", "float4", 2, 4, 1, 1, (4, 5), None, (0, 1)),
    ("1x9-up", "float4", 1, 4, 1, 9, (3, 20), None, (0, 1)),
    ("x2-c64", "x2", 2, 64, 7, 9, None, 2, (0,)),
    ("x2-c32-slice", "x2", 1, 32, 13, 5, None, 2, (0,)),                      # into channels [8, 40) of pitch 40
    ("x2-rows", "x2", 1, 4, 65540, 1, None, 2, (0,)),                         # n * ih > 65535 grid rows
    ("float4-rows", "x2", 1, 4, 131075, 1, (262150, 2), None, (0, 1)),        # n * oh > 4 * 65535
)
RESIZE_CROP = (2, 3, 12, 10)       # (top, left, full h, full w) of "nhwc-crop-to-nchw"
RESIZE_RUNS = [(i, m) for i, c in enumerate(RESIZE_CASES) for m in c[8]]
RESIZE_IDS = [f"{RESIZE_CASES[i][0]}-{('bilinear', 'nearest')[m]}" for i, m in RESIZE_RUNS]


def resize_out_hw(case):
    _, _, _, _, ih, iw, size, sf, _ = case
    return size if size is not None else (int(ih * sf), int(iw * sf))


def resize_scales(case, mode: int):
    """(scale_h, scale_w) as ops.resize passes them to the kernel."""
    from s2v_amd import ops
    _, _, _, _, ih, iw, _, sf, _ = case
    oh, ow = resize_out_hw(case)
    if mode == 0:
        return ops.torch_bilinear_scale(ih, oh, sf), ops.torch_bilinear_scale(iw, ow, sf)
    return (f32(1.0 / sf), f32(1.0 / sf)) if sf else (f32(ih / oh), f32(iw / ow))


@functools.lru_cache(maxsize=None)
def resize_case(i: int, mode: int):
    """x [n, c, ih, iw] float32 and the references [n, c, oh, ow]: bilinear ref64 / ref32 (F.interpolate in
    float32) / tolerance; nearest ``exact`` (F.interpolate mode='nearest')."""
    case = RESIZE_CASES[i]
    name, _, n, c, ih, iw, size, sf, _ = case
    oh, ow = resize_out_hw(case)
    x = rand(n, c, ih, iw, seed=4000 + i)
    if name == "nhwc-crop-to-nchw":      # the window of the full image: the values the kernel may not read differ
        t, l, fh, fw = RESIZE_CROP
        full = rand(n, c, fh, fw, seed=4000 + i)
        x = full[:, :, t:t + ih, l:l + iw].contiguous()
    else:
        full = None
    kw = dict(size=size) if size is not None else dict(scale_factor=sf)
    sh, sw = resize_scales(case, mode)
    d = dict(name=name, x=x, full=full, oh=oh, ow=ow, sh=sh, sw=sw, sf=sf)
    if mode == 0:
        ref64 = bilinear_ref64(x, oh, ow, sh, sw)
        ref32 = F.interpolate(x, mode="bilinear", align_corners=False, **kw)
        tol, e_ref, floor = tolerance(ref64, ref32)
        d.update(ref64=ref64, ref32=ref32, tol=tol, e_ref=e_ref, floor=floor)
    else:
        d.update(exact=F.interpolate(x, mode="nearest", **kw))
    return d


# ----------------------------------------------------------------------------- pad_reflect
PAD_NHW = (2, 9, 7)
PAD_PADS = ((0, 3, 2, 0), (PAD_NHW[1] - 1, 0, 0, PAD_NHW[2] - 1), (0, 0, 0, 0), (1, 1, 1, 1))    # (pt, pb, pl, pr)
# (name, c, x view, y view, kernel)
PAD_LAYOUTS = (
    ("c3", 3, (3, 0), (3, 0), "scalar"),
    ("c8-dense", 8, (8, 0), (8, 0), "float4"),
    ("c8-slices", 8, (16, 4), (20, 8), "float4"),
    ("c8-misaligned", 8, (12, 2), (8, 0), "scalar"),
)
PAD_RUNS = [(li, pi) for li in range(len(PAD_LAYOUTS)) for pi in range(len(PAD_PADS))]
PAD_IDS = [f"{PAD_LAYOUTS[li][0]}-" + ".".join(map(str, PAD_PADS[pi])) for li, pi in PAD_RUNS]


@functools.lru_cache(maxsize=None)
def pad_case(li: int, pi: int):
    """x [n, h, w, c] float32 and F.pad(mode='reflect') of it, NHWC."""
    c = PAD_LAYOUTS[li][1]
    pt, pb, pl, pr = PAD_PADS[pi]
    x = rand(*PAD_NHW, c, seed=5000 + li)
    exact = F.pad(x.permute(0, 3, 1, 2), (pl, pr, pt, pb), mode="reflect").permute(0, 2, 3, 1).contiguous()
    return dict(x=x, exact=exact)


# ----------------------------------------------------------------------------- row_pack
# (name, n, h, w, c, kw, pw, ycs, x view)
PACK_CASES = (
    ("c3-k7", 2, 3, 9, 3, 7, 3, 32, (3, 0)),
    ("c6-k7-narrow", 2, 3, 4, 6, 7, 3, 64, (6, 0)),           # a row narrower than the filter
    ("c5-k3-slice", 2, 3, 6, 5, 3, 0, 16, (8, 2)),
    ("c3-k7-narrow-slice", 1, 2, 4, 3, 7, 3, 32, (6, 3)),
)


def row_pack_ref(x: torch.Tensor, kw: int, pw: int, ycs: int) -> torch.Tensor:
    """y[n, h, w, dx * c + ci] = x[n, h, w + dx - pw, ci], +0.0 outside the row and in channels [kw * c,
    ycs): a plain index loop."""
    n, h, w, c = x.shape
    y = torch.zeros(n, h, w, ycs)
    for ox in range(w):
        for dx in range(kw):
            ix = ox + dx - pw
            if 0 <= ix < w:
                y[:, :, ox, dx * c:(dx + 1) * c] = x[:, :, ix]
    return y


@functools.lru_cache(maxsize=None)
def pack_case(i: int):
    _, n, h, w, c, kw, pw, ycs, _ = PACK_CASES[i]
    x = rand(n, h, w, c, seed=6000 + i)
    return dict(x=x, exact=row_pack_ref(x, kw, pw, ycs))


def bits(t: torch.Tensor) -> torch.Tensor:
    """The int32 bit patterns of a float32 tensor (so that -0.0 differs from +0.0)."""
    return t.contiguous().view(torch.int32)
