"""Inputs, fp64 references and bounds for the direct tests of the FIR resampler of csrc/fir.hip (``ops.fir2d``,
with the GPEN plane kernel of csrc/misc.hip behind ``torch_ops.upfirdn2d``) and the separable real DFTs of
csrc/fft.hip (``ops.rfft2`` / ``ops.irfft2``): pure CPU torch, shared by tests/test_fir_fft_direct_gpu.py (which
runs the kernels) and tests/test_fir_fft_cases_host.py (which checks that the tables reach the kernels they are
listed for and that the bounds tell a wrong kernel from a right one).

FIR.  The reference is upfirdn2d written out in float64 (``upfirdn_ref``): zero-insert ``up``, pad (a negative
pad crops), depthwise F.conv2d with the flipped kernel, every ``down``-th sample, then ``post * act(gain * fir +
bias[c])``.  The output size is the case's own: the far pad is whatever that size needs, so an output taller or
wider than upfirdn2d's reads zeros past the input.  Bound, per element:

    bound = K_FIR * 2^-24 * post * (|gain| * sum|x * k| + |bias|) + 2^-126

(the activations are at most 1-Lipschitz: the bound holds behind them).  K_FIR is the smallest power of two for
which two CPU float32 evaluations stay within half the bound on every element of every case: F.conv2d in
float32 with a float32 epilogue, and the kernel's own tap order (filter row, then column) as a chain of fmas
(``norm_cases.fma32``) with ``fma(gain, acc, bias)`` behind it.

    K_FIR = 8.  Worst err / bound with K = 8 over the fir2d and the plane cases: conv2d form and fma chain both
    0.486 (plane ``down2-negp1-16x65``; the CPU's depthwise conv2d sums in the same order on most elements);
    over the fir2d cases alone 0.364 / 0.305 (``blur4-sym-6x10-p2.2-o7x11``).  With K = 4 the plane case and
    the blur case are above one half.  (tests/test_fir_fft_cases_host.py recomputes both and fails if K is
    no longer the smallest.)

The exact set (inputs and bias multiples of 1/8 in [-1, 1], GPEN's [1 3 3 1] x [1 3 3 1] / 64 filter, times 4
for up2, gain = post = 1) has every product and partial sum representable in float32: the output must equal
the float64 reference bit for bit.

FFT.  The reference is the two separable passes in float64 with the float32 tables of ``ops.fft_tables(h, w,
"cpu")`` (the kernels' own operands: the rounding of the tables is not charged to the kernel).  Bound, per
element, with B the same two passes on the absolute values of every table entry and every input (+ |res|):

    bound = K_FFT * 2^-24 * B + 2^-126

K_FFT is found as K_FIR is, from the two passes as float32 matrix products (ffc_cases.rfft32 / irfft32 for
H != W) and as k-ordered chains of fmas in the generic kernels' order.

    K_FFT = 16.  Worst err / bound with K = 16: forward 0.261 in both forms (``mf48-n8-c8-offset``), inverse
    0.262 in both forms (``g40x56-offset``); with K = 8 all four are above one half.  The offset set decides
    it: every term of its DC sums has one sign, so the roundings of a chain do not cancel; the unit set stays
    at 0.101, the impulse set at 0.135.

Value sets of the FFT cases: "unit" U[-1, 1); "offset" 30 + U[-0.5, 0.5) (the DC bin is about h * w / 2 times
the others, which a max-norm tolerance would lose); "impulse" one nonzero sample per (image, channel) at a
position and with an amplitude that differ for every pair, so that every output is a single product chain
that carries the image, the channel and the position.

irfft2 accepts a misaligned ``y`` and ``res`` (the entry point asks 16-byte alignment of the spectrum alone):
the (C + 3, 1) and (C + 5, 2) slices are run, not refused.
"""
import functools
import math

import torch
import torch.nn.functional as F

import s2v_import  # noqa: F401
from ffc_cases import eighths, transform_tol  # noqa: F401
from misc_cases import EPS24, act_ref, f32, rand
from norm_cases import TINY, aligned, bits, fma32  # noqa: F401
from s2v_amd import ops
from s2v_amd._lib import ACT_LRELU, ACT_NONE, ACT_RELU

K_FIR = 8
K_FFT = 16
FIR_N = 2


# ----------------------------------------------------------------------------- FIR: the operation
def pad_crop(z: torch.Tensor, top: int, bottom: int, left: int, right: int) -> torch.Tensor:
    """Zero-pad the last two dimensions; a negative amount crops."""
    z = F.pad(z, [max(left, 0), max(right, 0), max(top, 0), max(bottom, 0)])
    return z[..., max(-top, 0):z.shape[-2] - max(-bottom, 0), max(-left, 0):z.shape[-1] - max(-right, 0)]


def upsampled(x: torch.Tensor, kh: int, kw: int, up: int, down: int, py0: int, px0: int, oh: int, ow: int,
              insert_zeros=True) -> torch.Tensor:
    """Steps 1 and 2 of upfirdn2d on x [n, c, h, w]: the zero-inserted image, padded (cropped) to the
    (oh - 1) * down + kh rows and (ow - 1) * down + kw columns an oh x ow output reads.  ``insert_zeros=False``
    repeats every sample instead (a host-test mutant: the zero-insertion test dropped)."""
    n, c, h, w = x.shape
    if insert_zeros:
        z = x.new_zeros(n, c, h * up, w * up)
        z[:, :, ::up, ::up] = x
    else:
        z = x.repeat_interleave(up, 2).repeat_interleave(up, 3)
    need_h, need_w = (oh - 1) * down + kh, (ow - 1) * down + kw
    z = pad_crop(z, py0, need_h - h * up - py0, px0, need_w - w * up - px0)
    assert z.shape[-2:] == (need_h, need_w), (z.shape, need_h, need_w)
    return z


def upfirdn_ref(x: torch.Tensor, k: torch.Tensor, up: int, down: int, py0: int, px0: int, oh: int, ow: int,
                flip=True, insert_zeros=True) -> torch.Tensor:
    """upfirdn2d of x [n, c, h, w] to [n, c, oh, ow] in x's dtype.  ``flip=False``: the host test's unflipped
    filter."""
    c = x.shape[1]
    kh, kw = k.shape
    z = upsampled(x, kh, kw, up, down, py0, px0, oh, ow, insert_zeros)
    wgt = (torch.flip(k, [0, 1]) if flip else k).to(x.dtype)[None, None].expand(c, 1, kh, kw).contiguous()
    return F.conv2d(z, wgt, groups=c)[:, :, ::down, ::down]


def fir_chain32(x: torch.Tensor, k: torch.Tensor, up: int, down: int, py0: int, px0: int, oh: int, ow: int):
    """The same sum as the kernels form it: acc = fma(x_tap, k_tap, acc) over the filter rows, then columns, in
    float32.  A tap outside the image or between two samples is a zero here and skipped there: the same acc."""
    kh, kw = k.shape
    z = upsampled(x, kh, kw, up, down, py0, px0, oh, ow)
    kf = torch.flip(k, [0, 1])
    acc = torch.zeros(x.shape[0], x.shape[1], oh, ow)
    for ti in range(kh):
        for tj in range(kw):
            tap = z[:, :, ti:ti + (oh - 1) * down + 1:down, tj:tj + (ow - 1) * down + 1:down]
            acc = fma32(tap, kf[ti, tj], acc)
    return acc


def own_size(size: int, up: int, p0: int, p1: int, k: int, down: int) -> int:
    """upfirdn2d's own output size."""
    return (size * up + p0 + p1 - k) // down + 1


# ----------------------------------------------------------------------------- FIR: the case table
# (bias, gain, post, act, alpha): no bias, then gain 1.5 and post sqrt(2) with each activation
EPILOGUES = (
    dict(bias=None, gain=1.0, post=1.0, act=ACT_NONE, alpha=0.0),
    dict(bias="own", gain=1.5, post=math.sqrt(2.0), act=ACT_NONE, alpha=0.0),
    dict(bias="own", gain=1.5, post=math.sqrt(2.0), act=ACT_LRELU, alpha=0.2),
    dict(bias="own", gain=1.5, post=math.sqrt(2.0), act=ACT_RELU, alpha=0.0),
)
FIR_KERNELS = ("blur4", "up2", "down2", "generic", "scalar")
SLICES = ((16, 4), (20, 8))          # the x and the y view of the sliced float4 cases (c = 8)


def _fir_cases():
    """kernel: the kernel a case is listed for (fir2d_blur4_rows; fir2d_kernel<true,2,1,4>, <true,1,2,4>,
    <true>, <false>).  A view is (pitch, channel offset); the epilogues cycle per kernel, the dense / sliced
    views of the float4 kernels alternate against them."""
    cases, count = [], {}

    def add(kernel, tag, ih, iw, oh, ow, pad0, *, kh=4, kw=4, up=1, down=1, c=8, x=None, y=None, bias=None,
            values="rand"):
        j = count.get(kernel, 0)
        count[kernel] = j + 1
        if values == "exact":
            e = dict(bias="own", gain=1.0, post=1.0, act=ACT_NONE, alpha=0.0)
        elif bias == "offset":
            e = dict(EPILOGUES[1 + j % 3], bias="offset")
        else:
            e = dict(EPILOGUES[j % 4])
        if kernel != "scalar" and x is None and (j + j // 4) % 2:
            x, y = SLICES
        cases.append(dict(
            name=f"{kernel}-{tag}-{ih}x{iw}-p{pad0[0]}.{pad0[1]}-o{oh}x{ow}", kernel=kernel, n=FIR_N, c=c, ih=ih, iw=iw,
            oh=oh, ow=ow, kh=kh, kw=kw, up=up, down=down, pad0=pad0, x=x or (c, 0), y=y or (c, 0), values=values, **e))

    # fir2d_blur4_rows: upfirdn2d pads (2, 2) and (1, 1): oh = h + 1 and h - 1, so 1, 2, 3 (shorter than a
    # strip) and every oh % 4; the last strip's input rows end past ih
    for j, h in enumerate((1, 2, 3, 4, 5, 6, 13)):
        for p, w in ((2, (1, 2, 10)[j % 3]), (1, (2, 10)[j % 2])):
            oh, ow = own_size(h, 1, p, p, 4, 1), own_size(w, 1, p, p, 4, 1)
            if oh > 0:
                add("blur4", "sym", h, w, oh, ow, (p, p))
    add("blur4", "asym", 5, 10, 5, 10, (2, 1))
    add("blur4", "asym", 5, 10, 5, 10, (0, 3))
    add("blur4", "asym", 13, 10, 13, 10, (0, 3))
    add("blur4", "neg", 5, 10, 3, 8, (-1, 0))
    add("blur4", "tall", 5, 10, 9, 13, (2, 1))           # 4 rows and 3 columns more than upfirdn2d's own
    add("blur4", "tall-neg", 6, 7, 8, 9, (-1, -2))
    # up2: the ToRGB upsample (pad0 (2, 2), 2h x 2w), and (1, 2)
    for h, w in ((5, 7), (1, 1)):
        add("up2", "torgb", h, w, 2 * h, 2 * w, (2, 2), up=2)
        add("up2", "asym", h, w, 2 * h + 1, 2 * w, (1, 2), up=2)
    # down2
    for h, w in ((10, 10), (9, 7)):
        add("down2", "sym", h, w, own_size(h, 1, 1, 1, 4, 2), own_size(w, 1, 1, 1, 4, 2), (1, 1), down=2)
        add("down2", "asym", h, w, own_size(h, 1, 2, 1, 4, 2), own_size(w, 1, 0, 2, 4, 2), (2, 0), down=2)
    # the runtime-generic float4 kernel
    add("generic", "k3x3", 6, 5, 6, 5, (1, 1), kh=3, kw=3)
    add("generic", "k1x4", 6, 5, 6, 5, (0, 2), kh=1, kw=4)
    add("generic", "k4x1", 6, 5, 6, 5, (1, 0), kh=4, kw=1)
    add("generic", "k5x2-up2", 6, 5, 12, 9, (3, -1), kh=5, kw=2, up=2)
    add("generic", "k8x8", 6, 5, 6, 5, (4, 3), kh=8, kw=8)
    add("generic", "up3", 5, 4, 15, 12, (2, 1), up=3)
    add("generic", "up2-down2", 7, 6, 7, 6, (1, 2), up=2, down=2)
    add("generic", "up2-down3", 7, 6, 5, 4, (2, 0), up=2, down=3)
    add("generic", "k3x3-tall", 4, 4, 7, 6, (-1, 1), kh=3, kw=3)
    # the scalar kernel: by channel count, by a misaligned x, by a misaligned y, by a misaligned bias; each at
    # the blur, up2, down2 and a generic form
    forms = (("blur", 5, 6, 5, 6, (2, 1), {}), ("up2", 3, 4, 6, 8, (2, 1), dict(up=2)),
             ("down2", 9, 7, 4, 4, (1, 2), dict(down=2)),
             ("k5x2-up3-down2", 4, 5, 6, 8, (2, 1), dict(kh=5, kw=2, up=3, down=2)))
    for lay, kw in (("c3", dict(c=3)), ("xmis", dict(x=(12, 2))), ("ymis", dict(y=(9, 1))), ("boff", dict(bias="offset"))):
        for tag, ih, iw, oh, ow, pad0, form in forms:
            add("scalar", f"{lay}-{tag}", ih, iw, oh, ow, pad0, **kw, **form)
    # the exact set: GPEN's filter, through blur4_rows, up2, down2 and the scalar kernel
    add("blur4", "exact", 6, 10, 6, 10, (2, 1), values="exact")
    add("up2", "exact", 5, 7, 10, 14, (2, 2), up=2, values="exact")
    add("down2", "exact", 10, 10, 5, 5, (1, 1), down=2, values="exact")
    add("scalar", "exact-c3", 6, 10, 6, 10, (2, 1), c=3, values="exact")
    return tuple(cases)


FIR_CASES = _fir_cases()
FIR_IDS = [s["name"] for s in FIR_CASES]


def gpen_filter(up: int) -> torch.Tensor:
    k = torch.tensor([1.0, 3.0, 3.0, 1.0])
    return k[None] * k[:, None] / 64 * (up * up)


def fir_eval(x, k, bias, s):
    """x [n, h, w, c], k [kh, kw], bias [c] or None (float32), s a dict with up / down / pad0 / oh / ow / gain /
    post / act / alpha -> NHWC results: ref64, unit (the bound in K = 1 units), conv32 and fma32."""
    args = (s["up"], s["down"], s["pad0"][0], s["pad0"][1], s["oh"], s["ow"])
    gain, post, alpha = f32(s["gain"]), f32(s["post"]), f32(s["alpha"])
    xc = x.permute(0, 3, 1, 2)
    b64 = bias.double()[None, :, None, None] if bias is not None else 0.0
    b32 = bias[None, :, None, None] if bias is not None else torch.zeros(1)
    fir64 = upfirdn_ref(xc.double(), k.double(), *args)
    ref64 = post * act_ref(gain * fir64 + b64, s["act"], alpha)
    mag = abs(gain) * upfirdn_ref(xc.double().abs(), k.double().abs(), *args, flip=True)
    unit = EPS24 * abs(post) * (mag + (bias.double().abs()[None, :, None, None] if bias is not None else 0.0))
    g32, p32 = torch.tensor(gain, dtype=torch.float32), torch.tensor(post, dtype=torch.float32)
    conv32 = p32 * act_ref(g32 * upfirdn_ref(xc, k, *args) + b32, s["act"], alpha)
    chain = fir_chain32(xc, k, *args)
    chain32 = p32 * act_ref(fma32(g32, chain, b32.expand_as(chain)), s["act"], alpha)
    nhwc = lambda t: t.permute(0, 2, 3, 1).contiguous()           # noqa: E731
    return dict(ref64=nhwc(ref64), unit=nhwc(unit), conv32=nhwc(conv32), fma32=nhwc(chain32))


@functools.lru_cache(maxsize=None)
def fir_case(i: int):
    """FIR_CASES[i]: x [n, ih, iw, c], k, bias (None, or elements [1, 1 + c) of ``bias_full``), the fp64
    reference [n, oh, ow, c], its bound unit and the two float32 evaluations."""
    s = FIR_CASES[i]
    shape = (s["n"], s["ih"], s["iw"], s["c"])
    if s["values"] == "exact":
        x, k = eighths(*shape, seed=8000 + i), gpen_filter(s["up"])
        full = eighths(s["c"] + 4, seed=8200 + i)
    else:
        x, k = rand(*shape, seed=8000 + i), rand(s["kh"], s["kw"], seed=8100 + i)
        full = rand(s["c"] + 4, seed=8200 + i)
    bias = full[1:1 + s["c"]].clone() if s["bias"] is not None else None
    d = fir_eval(x, k, bias, s)
    d.update(spec=s, x=x, k=k, bias=bias, bias_full=full)
    return d


def fir_bound(d) -> torch.Tensor:
    return K_FIR * d["unit"] + TINY


# ----------------------------------------------------------------------------- the GPEN plane kernel
# torch_ops.upfirdn2d on NCHW, pad = (p0, p1) on both axes, the output upfirdn2d's own: sizes on both sides of
# the 16 x 64 tile of upfirdn2d_plane4; a negative pad takes upfirdn2d_kernel.
# (name, kernel, up, down, (p0, p1), h, w)
PLANE_CASES = (
    ("blur-16x64", "plane4", 1, 1, (2, 1), 16, 64),
    ("blur-17x65", "plane4", 1, 1, (1, 2), 17, 65),
    ("blur-17x64", "plane4", 1, 1, (0, 3), 17, 64),
    ("up2-16x64", "plane4", 2, 1, (2, 1), 8, 32),
    ("up2-17x65", "plane4", 2, 1, (1, 3), 8, 32),
    ("down2-16x64", "plane4", 1, 2, (2, 1), 31, 127),
    ("down2-17x65", "plane4", 1, 2, (0, 3), 33, 129),
    ("down2-16x65", "plane4", 1, 2, (0, 2), 32, 130),
    ("blur-neg-17x65", "generic", 1, 1, (-1, 2), 19, 67),
    ("up2-neg-16x64", "generic", 2, 1, (-1, 4), 8, 32),
    ("down2-negp1-16x65", "plane4", 1, 2, (3, -2), 33, 131),
    ("down2-neg-16x65", "generic", 1, 2, (-2, 3), 33, 131),
)
PLANE_NC = (2, 3)


def plane_out_hw(case):
    _, _, up, down, (p0, p1), h, w = case
    return own_size(h, up, p0, p1, 4, down), own_size(w, up, p0, p1, 4, down)


@functools.lru_cache(maxsize=None)
def plane_case(i: int):
    """x [n, c, h, w], a random 4x4 filter, and NCHW ref64 / unit / conv32 / fma32."""
    _, _, up, down, (p0, _), h, w = PLANE_CASES[i]
    oh, ow = plane_out_hw(PLANE_CASES[i])
    x, k = rand(*PLANE_NC, h, w, seed=8500 + i), rand(4, 4, seed=8600 + i)
    args = (up, down, p0, p0, oh, ow)
    return dict(x=x, k=k, oh=oh, ow=ow, ref64=upfirdn_ref(x.double(), k.double(), *args),
                unit=EPS24 * upfirdn_ref(x.double().abs(), k.double().abs(), *args),
                conv32=upfirdn_ref(x, k, *args), fma32=fir_chain32(x, k, *args))


# ----------------------------------------------------------------------------- FFT: the operation
def tables(h: int, w: int):
    """(fw [w, 2, wf], fh [h, 2, u], ih [u, 2, h], iw [wf, 2, w]) float32: the kernels' operands."""
    wf = w // 2 + 1
    t = ops.fft_tables(h, w, "cpu")
    fw, t = t[:2 * wf * w].reshape(w, 2, wf), t[2 * wf * w:]
    fh, t = t[:2 * h * h].reshape(h, 2, h), t[2 * h * h:]
    ih, t = t[:2 * h * h].reshape(h, 2, h), t[2 * h * h:]
    return fw, fh, ih, t.reshape(wf, 2, w)


def to_spec(zr: torch.Tensor, zi: torch.Tensor) -> torch.Tensor:
    """[n, h, wf, c] real and imaginary parts -> the spectrum layout [n, h * wf, 2c], channel part * c + c."""
    n, h, wf, c = zr.shape
    return torch.cat([zr, zi], -1).reshape(n, h * wf, 2 * c)


def from_spec(sp: torch.Tensor, h: int):
    n, f, c2 = sp.shape
    z = sp.reshape(n, h, f // h, c2)
    return z[..., :c2 // 2], z[..., c2 // 2:]


def rfft_passes(x: torch.Tensor, dtype=torch.float64, absolute=False, h_sign=-1.0) -> torch.Tensor:
    """x [n, h, w, c] -> [n, h * wf, 2c]: the W pass (real -> half spectrum) and the complex H pass as matrix
    products in ``dtype``.  ``absolute``: every table entry and input by its absolute value, every sign plus
    (the bound's B).  ``h_sign=+1``: the host test's wrong sign of fi in the H pass."""
    n, h, w, c = x.shape
    fw, fh, _, _ = (t.to(dtype) for t in tables(h, w))
    x = x.to(dtype)
    if absolute:
        fw, fh, x, h_sign = fw.abs(), fh.abs(), x.abs(), 1.0
    y = torch.einsum("wpv,nhwc->pnhvc", fw, x)
    fr, fi = fh[:, 0], fh[:, 1]
    zr = torch.einsum("hu,nhvc->nuvc", fr, y[0]) + h_sign * torch.einsum("hu,nhvc->nuvc", fi, y[1])
    zi = torch.einsum("hu,nhvc->nuvc", fr, y[1]) + torch.einsum("hu,nhvc->nuvc", fi, y[0])
    return to_spec(zr, zi)


def irfft_passes(sp: torch.Tensor, h: int, w: int, res=None, dtype=torch.float64, absolute=False, iw=None):
    """sp [n, h * wf, 2c] -> [n, h, w, c]: the complex inverse H pass and the c2r W pass (+ res).  ``iw``:
    another c2r table (the host test's mutant)."""
    _, _, ih, iw_ = (t.to(dtype) for t in tables(h, w))
    iw = iw_ if iw is None else iw.to(dtype)
    zr, zi = from_spec(sp.to(dtype), h)
    g_sign = -1.0
    if absolute:
        ih, iw, zr, zi, g_sign = ih.abs(), iw.abs(), zr.abs(), zi.abs(), 1.0
    gr, gi = ih[:, 0], ih[:, 1]
    yr = torch.einsum("uh,nuvc->nhvc", gr, zr) + g_sign * torch.einsum("uh,nuvc->nhvc", gi, zi)
    yi = torch.einsum("uh,nuvc->nhvc", gr, zi) + torch.einsum("uh,nuvc->nhvc", gi, zr)
    y = torch.einsum("vw,nhvc->nhwc", iw[:, 0], yr) + torch.einsum("vw,nhvc->nhwc", iw[:, 1], yi)
    if res is not None:
        y = y + (res.to(dtype).abs() if absolute else res.to(dtype))
    return y


def rfft_chain32(x: torch.Tensor) -> torch.Tensor:
    """rfft2_kernel's arithmetic: per output one chain of fmas over w, then over h."""
    n, h, w, c = x.shape
    fw, fh, _, _ = tables(h, w)
    wf = w // 2 + 1
    re, im = torch.zeros(n, h, wf, c), torch.zeros(n, h, wf, c)
    for k in range(w):
        xv = x[:, :, k, None, :]
        re = fma32(fw[k, 0][None, None, :, None], xv, re)
        im = fma32(fw[k, 1][None, None, :, None], xv, im)
    zr, zi = torch.zeros(n, h, wf, c), torch.zeros(n, h, wf, c)
    for k in range(h):
        yr, yi = re[:, k, None], im[:, k, None]
        fr, fi = fh[k, 0][None, :, None, None], fh[k, 1][None, :, None, None]
        zr = fma32(fr, yr, fma32(-fi, yi, zr))
        zi = fma32(fi, yr, fma32(fr, yi, zi))
    return to_spec(zr, zi)


def irfft_chain32(sp: torch.Tensor, h: int, w: int, res=None) -> torch.Tensor:
    """irfft2_kernel's arithmetic: chains of fmas over u, then over v (real and imaginary term per step), the
    residual added last."""
    _, _, ih, iw = tables(h, w)
    zr, zi = from_spec(sp, h)
    n, _, wf, c = zr.shape
    yr, yi = torch.zeros(n, h, wf, c), torch.zeros(n, h, wf, c)
    for k in range(h):
        ar, ai = zr[:, k, None], zi[:, k, None]
        gr, gi = ih[k, 0][None, :, None, None], ih[k, 1][None, :, None, None]
        yr = fma32(gr, ar, fma32(-gi, ai, yr))
        yi = fma32(gi, ar, fma32(gr, ai, yi))
    acc = torch.zeros(n, h, w, c)
    for k in range(wf):
        acc = fma32(iw[k, 0][None, None, :, None], yr[:, :, k, None, :],
                    fma32(iw[k, 1][None, None, :, None], yi[:, :, k, None, :], acc))
    return acc if res is None else acc + res


# ----------------------------------------------------------------------------- FFT: the case table
FFT_VALUES = ("unit", "offset", "impulse")


def _fft(name, kernel, n, c, h, w, *, x="dense", extra=0, res=None, y="dense"):
    """kernel "mfma" (rfft2_mf / irfft2_mf) or "generic" (rfft2_kernel / irfft2_kernel); x "dense" or "slice"
    (channels [4, 4 + C) of pitch C + 4); extra: spectrum pitch 2C + extra; res None, "dense" or "slice" ((C +
    5, 2)); y "dense" or "slice" ((C + 3, 1))."""
    return dict(name=name, kernel=kernel, n=n, c=c, h=h, w=w, x=(c, 0) if x == "dense" else (c + 4, 4), scs=2 * c + extra,
                res=None if res is None else (c, 0) if res == "dense" else (c + 5, 2),
                y=(c, 0) if y == "dense" else (c + 3, 1))


FFT_CASES = (
    # H = W in {12, 24, 48}: n in {8, 16} takes the XCD permutation of fft_block (one, two and three channel
    # groups per image), the others the plain order
    _fft("mf12-n3-c8", "mfma", 3, 8, 12, 12, x="slice", res="dense"),
    _fft("mf12-n8-c4", "mfma", 8, 4, 12, 12, extra=8, y="slice"),
    _fft("mf12-n8-c12", "mfma", 8, 12, 12, 12, x="slice", extra=8, res="slice"),
    _fft("mf12-n16-c8", "mfma", 16, 8, 12, 12, res="slice", y="slice"),
    _fft("mf24-n3-c8", "mfma", 3, 8, 24, 24, extra=8, res="slice", y="slice"),
    _fft("mf24-n8-c8", "mfma", 8, 8, 24, 24, x="slice"),
    _fft("mf48-n1-c4", "mfma", 1, 4, 48, 48, x="slice", extra=8, res="dense", y="slice"),
    _fft("mf48-n8-c8", "mfma", 8, 8, 48, 48, res="slice"),
    # the generic kernels: W != H, odd sizes (no Nyquist column), H = 1, W = 2, an LNet height that is not
    # square, two channel groups per image, and tiles above the 64 KB of dynamic LDS a kernel gets unasked
    _fft("g6x10", "generic", 2, 4, 6, 10, x="slice", res="dense"),
    _fft("g5x7", "generic", 3, 4, 5, 7, extra=8, res="slice", y="slice"),
    _fft("g13x13", "generic", 2, 4, 13, 13, extra=8),
    _fft("g1x8", "generic", 2, 4, 1, 8, x="slice", res="slice"),
    _fft("g7x2", "generic", 2, 4, 7, 2, y="slice", res="dense"),
    _fft("g24x12", "generic", 2, 4, 24, 12, x="slice", extra=8, y="slice"),
    _fft("g13x13-c8", "generic", 2, 8, 13, 13, x="slice", extra=8, res="slice", y="slice"),
    _fft("g40x56", "generic", 1, 4, 40, 56, res="slice"),
    _fft("g56x56", "generic", 1, 4, 56, 56, x="slice", extra=8, y="slice"),
)
FFT_RUNS = [(i, v) for i in range(len(FFT_CASES)) for v in FFT_VALUES]
FFT_IDS = [f"{FFT_CASES[i]['name']}-{v}" for i, v in FFT_RUNS]


def _coprime_step(m: int) -> int:
    return next(p for p in (7, 11, 13, 17, 19, 23, 29, 31) if math.gcd(p, m) == 1)


def impulse(n: int, slots: int, c: int) -> torch.Tensor:
    """[n, slots, c] float32, zero but for one sample per (image, channel): pair q = image * c + channel has
    amplitude 1 + q / (n c) at slot (q * step) % slots, step coprime to slots (distinct while n c <= slots)."""
    assert n * c <= slots, "a slot for every (image, channel) pair"
    q = torch.arange(n * c)
    t = torch.zeros(n, slots, c)
    t[q // c, (q * _coprime_step(slots)) % slots, q % c] = (1.0 + q.double() / (n * c)).float()
    return t


def _fft_values(kind, n, slots, c, seed):
    if kind == "offset":
        return (30.0 + rand(n, slots, c, seed=seed, lo=-0.5, hi=0.5).double()).float()
    if kind == "impulse":
        return impulse(n, slots, c)
    return rand(n, slots, c, seed=seed)


@functools.lru_cache(maxsize=8)
def fft_case(i: int, values: str):
    """FFT_CASES[i] with a value set.  Forward: x [n, h, w, c], spec64 [n, F, 2c], spec_unit, spec_mm32 /
    spec_fma32.  Inverse: sp [n, F, 2c] (the impulse over the 2F (frequency, part) slots of a channel), res or
    None, y64 [n, h, w, c], y_unit, y_mm32 / y_fma32."""
    s = FFT_CASES[i]
    n, c, h, w = s["n"], s["c"], s["h"], s["w"]
    f = h * (w // 2 + 1)
    k = FFT_VALUES.index(values)
    x = _fft_values(values, n, h * w, c, 9000 + 10 * i + k).reshape(n, h, w, c)
    sp = _fft_values(values, n, 2 * f, c, 9300 + 10 * i + k).reshape(n, f, 2, c).reshape(n, f, 2 * c)
    res = rand(n, h, w, c, seed=9600 + 10 * i + k) if s["res"] is not None else None
    return dict(spec=s, values=values, x=x, sp=sp, res=res,
                spec64=rfft_passes(x), spec_unit=EPS24 * rfft_passes(x, absolute=True),
                spec_mm32=rfft_passes(x, dtype=torch.float32), spec_fma32=rfft_chain32(x),
                y64=irfft_passes(sp, h, w, res), y_unit=EPS24 * irfft_passes(sp, h, w, res, absolute=True),
                y_mm32=irfft_passes(sp, h, w, res, dtype=torch.float32), y_fma32=irfft_chain32(sp, h, w, res))


def fft_bound(unit: torch.Tensor) -> torch.Tensor:
    return K_FFT * unit + TINY


def xcd_order(n: int, groups: int):
    """fft_block(): the (image, channel group) of every block, in block order."""
    out = []
    for b in range(n * groups):
        if n % 8 == 0:
            idx = b >> 3
            out.append(((idx // groups) * 8 + (b & 7), idx % groups))
        else:
            out.append((b // groups, b % groups))
    return out
