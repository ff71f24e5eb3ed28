"""Direct fp64 parity of the small non-conv kernels of csrc/misc.hip and csrc/norm.hip, called through
``ops.*``: flow warp (+ cat), attention, token LayerNorm, eltwise and amax, at the shapes, views and
value ranges where they can go wrong (tests/misc_cases.py builds the inputs and references;
tests/test_misc_cases_host.py checks on the CPU that the inputs reach those paths).

Flow warp, attention and LayerNorm take their tolerance from the reference: with ``e_ref`` the error
of the same formula in fp32 on the CPU, ``max|got - ref64| <= max(4 * e_ref, 16 * 2^-24 * max|ref64|)``.
Eltwise has a per-element rounding bound, amax is exact.  Every output buffer and every padding
channel beside a sliced output is pre-filled with NaN: what the kernel must write has to come out
finite, what it must not touch has to stay NaN.  Run with ``-s`` to see e_ref and the achieved error
of every case.
"""
import pytest
import torch

import s2v_import  # noqa: F401

pytestmark = pytest.mark.gpu

import misc_cases as mc  # noqa: E402
from s2v_amd import ops  # noqa: E402
from s2v_amd.ops import NHWC  # noqa: E402

DEV = "cuda"
NAN = float("nan")


@pytest.fixture(scope="module")
def ctx():
    return ops.Ctx(DEV)


def nan_nhwc(n, h, w, pitch):
    return torch.full((n, h, w, pitch), NAN, device=DEV)


def put(values: torch.Tensor, pitch: int, off: int, fill=NAN) -> NHWC:
    """``values`` [N, H, W, c] as the channel slice [off, off + c) of a new [N, H, W, pitch] device
    tensor whose other channels hold ``fill``."""
    n, h, w, c = values.shape
    t = torch.full((n, h, w, pitch), fill, device=DEV)
    t[..., off:off + c] = values.to(DEV)
    return NHWC(t, off, c)


def check_canary(v: NHWC, what):
    """The channels of v's tensor outside the view are still NaN, the view itself is finite."""
    t = v.t.cpu()
    inside = torch.zeros(v.cs, dtype=torch.bool)
    inside[v.coff:v.coff + v.c] = True
    assert torch.isnan(t[..., ~inside]).all(), f"{what}: wrote outside its channel slice"
    assert torch.isfinite(t[..., inside]).all(), f"{what}: left part of its output unwritten or non-finite"


def check_close(got64, d, what):
    err = float((got64 - d["ref64"]).abs().max())
    print(f"{what}: e_ref={d['e_ref']:.2e} floor={d['floor']:.2e} tol={d['tol']:.2e} err={err:.2e}")
    assert torch.isfinite(got64).all(), what
    assert err <= d["tol"], f"{what}: err {err:.3e} > tol {d['tol']:.3e} (e_ref {d['e_ref']:.3e})"
    return err


# ----------------------------------------------------------------------------- flow warp
def warp_views(i, ycat=False):
    name, n, c, h, w, fh, fw, _, sform, fform, yform = mc.WARP_CASES[i]
    d = mc.warp_case(i)
    if sform == "nhwc":
        src = d["src"].permute(0, 2, 3, 1).contiguous().to(DEV).permute(0, 3, 1, 2)
        assert src.stride(1) == 1
    elif sform == "slice":
        wide = torch.full((n, c + 3, h, w), NAN, device=DEV)
        wide[:, 1:1 + c] = d["src"].to(DEV)
        src = wide[:, 1:1 + c]
    else:
        src = d["src"].to(DEV)
    fl = d["flow"].permute(0, 2, 3, 1)
    flow = put(fl, 4, 1) if fform == "slice" else put(fl, 2, 0)
    cy = 2 * c if ycat else c
    y = NHWC(nan_nhwc(n, h, w, cy + 5), 3, cy) if yform == "slice" or ycat else NHWC(nan_nhwc(n, h, w, cy))
    return d, flow, src, y


@pytest.mark.parametrize("i", range(len(mc.WARP_CASES)), ids=[c[0] for c in mc.WARP_CASES])
def test_flow_warp_fp64(ctx, i):
    """s2v_flow_warp against oracle.nets.warp_image in float64: non-square images, per-axis resize
    ratios, flow at image size, 1 / 10 / 12 / 16 blocks (the XCD remap with and without remainder), a
    ragged last block, NHWC / channel-sliced sources, flow and output as channel slices, samples far
    outside (the +-1e4 patch must give exactly 0), a band of samples with two taps outside.

    Measured on MI355X (e_ref / err): 16blk 3.32e-05 / 3.60e-05, same 4.42e-06 / 3.36e-06, 12full
    7.68e-06 / 7.89e-06, 1axis 7.41e-06 / 7.41e-06, tiny 7.10e-07 / 5.62e-07, patch 5.52e-06 / 5.52e-06."""
    d, flow, src, y = warp_views(i)
    ops.flow_warp(ctx, flow, src, y)
    torch.cuda.synchronize()
    check_canary(y, f"flow_warp {d['name']}")
    got = y.v.permute(0, 3, 1, 2).cpu()
    check_close(got.double(), d, f"flow_warp {d['name']}")
    if d["patch"] is not None:
        patch = d["patch"].expand_as(got)
        assert (got[patch] == 0).all(), "samples far outside the image must be exactly 0"


@pytest.mark.parametrize("i", range(len(mc.WARP_CASES)), ids=[c[0] for c in mc.WARP_CASES])
def test_flow_warp_cat(ctx, i):
    """s2v_flow_warp_cat writes [src | flow_warp(src)] into a 2c-channel slice of a wider tensor
    (ycs = 2c + 5): the copy half bit-equal to src, the warp half bit-equal to s2v_flow_warp's output
    on the same inputs, nothing beside the slice.  (Bit equality: no error figures.)"""
    d, flow, src, y = warp_views(i)
    _, _, _, ycat = warp_views(i, ycat=True)
    ops.flow_warp(ctx, flow, src, y)
    ops.flow_warp_cat(ctx, flow, src, ycat)
    torch.cuda.synchronize()
    check_canary(ycat, f"flow_warp_cat {d['name']}")
    c = d["src"].shape[1]
    got = ycat.v.permute(0, 3, 1, 2).cpu()
    assert torch.equal(got[:, :c], d["src"]), "copy half"
    assert torch.equal(got[:, c:], y.v.permute(0, 3, 1, 2).cpu()), "warp half differs from flow_warp"


# ----------------------------------------------------------------------------- attention
@pytest.mark.parametrize("i", range(len(mc.ATTN_CASES)),
                         ids=[f"b{b}-T{T}-h{h}-m{int(m)}" for b, T, h, m in mc.ATTN_CASES])
def test_attention_fp64(ctx, i):
    """s2v_attention against softmax(q k^T / 8) v in float64: T = 256 (LDS limit, 16 row groups), T =
    1 and 3 (waves without a row), T = 65, T = 200 with logits to +-208 (overflows without the row-max
    subtraction), batch * heads = 512 (one row group), a small row-group count; q and k are column
    halves of one tensor, v and out column slices of wider ones.

    Measured on MI355X (e_ref / err; where the floor 16 * 2^-24 * max|ref64| sets the tolerance it is
    given too): b1-T256-h2 6.37e-08 / 8.89e-08, b3-T1-h1 0 / 0 (floor 9.43e-07), b2-T3-h2 1.04e-07 /
    9.73e-08 (floor 8.22e-07), b2-T65-h3-m6 5.86e-06 / 5.77e-06, b1-T200-h1-m12 1.41e-05 / 1.41e-05,
    b64-T5-h8 1.43e-07 / 1.63e-07 (floor 8.77e-07), b2-T12-h1 8.30e-08 / 1.09e-07 (floor 5.48e-07).
    (e_ref of the matmul-based CPU reference moves in its last digits with the host's BLAS.)"""
    b, T, heads, _ = mc.ATTN_CASES[i]
    d = mc.attn_case(i)
    hc = heads * 64
    qk = torch.cat([d["q"], d["k"]], 1).to(DEV)
    vw = torch.full((b * T, hc + 7), NAN, device=DEV)
    vw[:, 5:5 + hc] = d["v"].to(DEV)
    ow = torch.full((b * T, hc + 6), NAN, device=DEV)
    ops.attention(ctx, qk[:, :hc], qk[:, hc:], vw[:, 5:5 + hc], ow[:, 2:2 + hc], batch=b, heads=heads, tokens=T)
    torch.cuda.synchronize()
    ow = ow.cpu()
    assert torch.isnan(ow[:, :2]).all() and torch.isnan(ow[:, 2 + hc:]).all(), "wrote outside its column slice"
    check_close(ow[:, 2:2 + hc].double(), d, f"attention {mc.ATTN_CASES[i]}")


def test_attention_rejects_unsupported_shapes(ctx):
    """tokens = 257 (beyond the 256-token score registers) and dim_head = 32 are errors."""
    def run(T, dh):
        t = torch.zeros(T, 4 * dh, device=DEV)
        ops.attention(ctx, t[:, :dh], t[:, dh:2 * dh], t[:, 2 * dh:3 * dh], t[:, 3 * dh:], batch=1, heads=1, tokens=T,
                      dim_head=dh)
    run(4, 64)
    with pytest.raises(RuntimeError, match="tokens <= 256"):
        run(257, 64)
    with pytest.raises(RuntimeError, match="dim_head 64"):
        run(4, 32)
    torch.cuda.synchronize()


# ----------------------------------------------------------------------------- token LayerNorm
@pytest.mark.parametrize("i", range(len(mc.LN_CASES)), ids=[f"{r}x{dm}-off{int(o)}" for r, dm, o, _ in mc.LN_CASES])
def test_row_layernorm_fp64(ctx, i):
    """s2v_row_layernorm against F.layer_norm in float64: rows % 4 != 0, dim < 64, dim % 64 != 0, dim =
    1 (the output is the bias), a mean 1000x / 5000x the spread, LNet's 288 x 512; x and y are column
    slices of wider tensors.

    Measured on MI355X (e_ref / err): 5x512-off1000 6.89e-05 / 5.56e-05, 7x100 2.95e-07 / 2.01e-07
    (floor 2.27e-06), 3x1 0 / 0 (floor 5.16e-07), 9x63-off50 6.12e-04 / 7.08e-04, 4x65 2.00e-07 /
    1.08e-07 (floor 2.28e-06), 288x512 4.08e-07 / 2.82e-07 (floor 2.47e-06)."""
    rows, dim, _, _ = mc.LN_CASES[i]
    d = mc.ln_case(i)
    xw = torch.full((rows, dim + 5), NAN, device=DEV)
    xw[:, 2:2 + dim] = d["x"].to(DEV)
    yw = torch.full((rows, dim + 3), NAN, device=DEV)
    ops.row_layernorm(ctx, xw[:, 2:2 + dim], d["w"].to(DEV), d["b"].to(DEV), yw[:, 1:1 + dim], eps=mc.LN_EPS)
    torch.cuda.synchronize()
    yw = yw.cpu()
    assert torch.isnan(yw[:, :1]).all() and torch.isnan(yw[:, 1 + dim:]).all(), "wrote outside its column slice"
    check_close(yw[:, 1:1 + dim].double(), d, f"row_layernorm {mc.LN_CASES[i]}")


# ----------------------------------------------------------------------------- eltwise
@pytest.mark.parametrize("i", range(len(mc.ELT_CASES)), ids=[c["name"] for c in mc.ELT_CASES])
def test_eltwise_fp64(ctx, i):
    """s2v_eltwise against post * act(x * a * mul + add + bias[c]) in float64, per element within 4 *
    2^-23 * (|x a mul| + |add| + |bias|) * |post| (none / relu / lrelu) or 8 * 2^-23 * (... + 1) *
    |post| (sigmoid / tanh / gelu): every mul / add / bias combination on the float4 layout (c = 8,
    aligned) and the scalar one (c = 6), the c = 8 layouts that must fall back to scalar, the six
    activations, in place on a channel slice (GFPGAN SFT), add = output (RRDB), 105 pixels.

    Measured on MI355X (largest err / bound per group; the CPU fp32 evaluation gives the same figures
    except tanh, 0.039 / 0.033): mul x add x bias 0.193 (float4) and 0.198 (scalar); scalar fall-backs
    0.223; none 0.259 / 0.234, relu 0.213 / 0.265, lrelu 0.261 / 0.211, sigmoid 0.054 / 0.048, tanh
    0.049 / 0.035, gelu_tanh 0.121 / 0.123 (float4 / scalar); in place 0.188; add = output 0.164.
    The largest absolute error is 8.5e-07 (b-gelu_tanh)."""
    d = mc.elt_case(i)
    s = d["spec"]
    x = put(d["x"], *s["x"])
    y = x if s["y"] == "x" else NHWC(nan_nhwc(*mc.ELT_NHW, s["y"][0]), s["y"][1], s["c"])
    mul = put(d["mul"], *s["mul"]) if s["mul"] is not None else None
    if s["add"] == "y":
        y.v.copy_(d["add"].to(DEV))
        add = y
    else:
        add = put(d["add"], *s["add"]) if s["add"] is not None else None
    bias = None
    if s["bias"] == "own":
        bias = d["bias"].to(DEV)
    elif s["bias"] == "offset":
        bias = torch.full((s["c"] + 4,), NAN, device=DEV)
        bias[1:1 + s["c"]] = d["bias"].to(DEV)
        bias = bias[1:1 + s["c"]]
        assert bias.data_ptr() % 16 == 4
    ops.eltwise(ctx, x, y, a=s["a"], mul=mul, add=add, bias=bias, act=d["act"], alpha=s["alpha"], post=s["post"])
    torch.cuda.synchronize()
    check_canary(y, f"eltwise {s['name']}")
    if y is not x:
        assert torch.equal(x.v.cpu(), d["x"]), "the input changed"
    err = (y.v.cpu().double() - d["ref64"]).abs()
    ratio = float((err / d["bound"]).max())
    cpu = float(((d["ref32"].double() - d["ref64"]).abs() / d["bound"]).max())
    print(f"eltwise {s['name']}: max err={float(err.max()):.2e} err/bound={ratio:.3f} (CPU fp32 {cpu:.3f})")
    assert ratio <= 1.0, f"eltwise {s['name']}: err / bound = {ratio:.3f}"


# ----------------------------------------------------------------------------- amax
def amax_of(view: torch.Tensor) -> torch.Tensor:
    out = torch.full((1,), NAN, device=DEV)
    ops._amax_into(view, out)
    torch.cuda.synchronize()
    return out.cpu()[0]


@pytest.mark.parametrize("i", range(len(mc.AMAX_CASES)), ids=[c[0] for c in mc.AMAX_CASES])
def test_amax_is_exact(ctx, i):
    """s2v_amax is bit-equal to t.abs().max(): one / three / 64 quads per row (an idle lane), the
    grid-stride loop past 2048 blocks in the float4 and the scalar form, 130 channels on 64 lanes, a
    misaligned 8-channel slice; the channels beside the view hold 1e6 and must not count.  The
    maximum sits at the first element, the last, the last channel of a middle pixel, and once negative.

    Measured on MI355X: all 24 placements return 3.5 exactly (a maximum has no rounding: e_ref = err = 0)."""
    name, nhw, c, pitch, off = mc.AMAX_CASES[i]
    pixels = nhw[0] * nhw[1] * nhw[2]
    base = mc.amax_base(i)
    dev = base.to(DEV)
    view, flat = dev[..., off:off + c], dev.view(pixels, pitch)
    ref0 = base[..., off:off + c].abs().max()
    assert torch.equal(amax_of(view), ref0), f"{name}: no peak"
    for place, sign in mc.AMAX_PLACEMENTS:
        p, ch = mc.amax_position(place, pixels, c)
        keep = flat[p, off + ch].clone()
        flat[p, off + ch] = sign * mc.AMAX_PEAK
        got = amax_of(view)
        flat[p, off + ch] = keep
        print(f"amax {name} {place}: {float(got)}")
        assert float(got) == mc.AMAX_PEAK, f"{name}: peak at {place} (pixel {p}, channel {ch}) gave {float(got)}"
    assert torch.equal(dev.cpu(), base), "the input changed"


@pytest.mark.parametrize("i", (1, 3), ids=["float4", "scalar"])
def test_amax_special_values(ctx, i):
    """An all-zero input gives exactly 0 (into an output that held NaN), one NaN gives NaN, a maximum
    of 70000 (above the f16 range) comes back as 70000."""
    name, nhw, c, pitch, off = mc.AMAX_CASES[i]
    pixels = nhw[0] * nhw[1] * nhw[2]
    dev = mc.amax_base(i).to(DEV)
    view, flat = dev[..., off:off + c], dev.view(pixels, pitch)
    p, ch = mc.amax_position("mid-lastch", pixels, c)
    flat[p, off + ch] = -70000.0
    assert float(amax_of(view)) == 70000.0
    flat[p, off + ch] = NAN
    assert torch.isnan(amax_of(view))
    flat[p, off + ch] = -NAN
    assert torch.isnan(amax_of(view))
    view.zero_()
    got = amax_of(view)
    assert float(got) == 0.0 and not torch.signbit(got)


def test_amax_into_2d_rows(ctx):
    """ops._amax_into on an [N, C] column slice of a wider matrix (the row view of the linear layers)."""
    n, c = 37, 20
    t = torch.full((n, c + 9), mc.AMAX_NEIGHBOUR)
    t[:, 3:3 + c] = mc.rand(n, c, seed=1100)
    for p, ch, val in ((0, 0, 2.5), (n - 1, c - 1, -4.25), (n // 2, c - 1, 3.0)):
        t[p, 3 + ch] = val
        out = torch.full((1,), NAN, device=DEV)
        ops._amax_into(t.to(DEV)[:, 3:3 + c], out)
        torch.cuda.synchronize()
        assert torch.equal(out.cpu()[0], t[:, 3:3 + c].abs().max())
