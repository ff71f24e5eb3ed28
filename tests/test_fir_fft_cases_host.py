"""CPU checks of the tables that tests/test_fir_fft_direct_gpu.py feeds the FIR and FFT kernels
(tests/fir_fft_cases.py): every case reaches the kernel it is listed for (the dispatch conditions of s2v_fir2d,
s2v_rfft2, s2v_irfft2 and upfirdn2d_t restated as predicates on shape, pitch and offset, their constants read
from the sources), the references state upfirdn2d and torch.fft's transforms, K_FIR and K_FFT are the smallest
powers of two that two CPU float32 evaluations keep within half the bound, and a deliberately wrong variant
of every kernel family lands outside its bound.  Run with ``-s`` for the figures."""
import os
import re

import torch

import fir_fft_cases as fc
import s2v_import

CSRC = os.path.join(s2v_import.PKG_DIR, "csrc")


def source(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def grab(text, pattern):
    m = re.search(pattern, text)
    assert m, f"the launch arithmetic changed: {pattern!r} is no longer in the source"
    return [int(g) for g in m.groups()]


FIR = source("fir.hip")
FFT = source("fft.hip")
MISC = source("misc.hip")
(FIR_MAX_TAPS,) = grab(FIR, r"constexpr int FIR_MAX_TAPS = (\d+);")
(FIR_BLUR_ROWS,) = grab(FIR, r"#define FIR_BLUR_ROWS (\d+)")
(FIR_ROWS,) = grab(FIR, r"constexpr int FIR_ROWS = (\d+);")
(FFT_LDS_KB,) = grab(FFT, r"\* sizeof\(float\) <= (\d+) \* 1024\) \? 4 : 0;")
FFT_MF_SIZES = tuple(grab(FFT, r"h == w && \(h == (\d+) \|\| h == (\d+) \|\| h == (\d+)\)"))
PLANE_TY, PLANE_TX = grab(MISC, r"constexpr int TY = (\d+), TX = (\d+);")


# ----------------------------------------------------------------------------- FIR: dispatch
def fir_kernel(s) -> str:
    """s2v_fir2d's choice.  The tensors are 16-byte aligned, so a pointer is aligned when its channel offset is
    a multiple of 4; bias "offset" starts one float into its tensor."""
    vec = (s["c"] % 4 == 0 and fc.aligned(s["x"]) and fc.aligned(s["y"]) and s["bias"] != "offset")
    k4 = s["kh"] == 4 and s["kw"] == 4
    if not vec:
        return "scalar"
    if k4 and (s["up"], s["down"]) == (1, 1):
        return "blur4" if FIR_BLUR_ROWS else "one-output blur"
    if k4 and (s["up"], s["down"]) == (2, 1):
        return "up2"
    if k4 and (s["up"], s["down"]) == (1, 2):
        return "down2"
    return "generic"


def of_kernel(kernel, values="rand"):
    return [s for s in fc.FIR_CASES if s["kernel"] == kernel and s["values"] == values]


def test_fir_cases_reach_their_kernels():
    assert (FIR_MAX_TAPS, FIR_BLUR_ROWS, FIR_ROWS) == (64, 1, 4)
    assert len(set(fc.FIR_IDS)) == len(fc.FIR_IDS)
    for s in fc.FIR_CASES:
        assert fir_kernel(s) == s["kernel"], s["name"]
        assert s["n"] == 2 and s["kh"] * s["kw"] <= FIR_MAX_TAPS and s["oh"] > 0 and s["ow"] > 0
        for view in (s["x"], s["y"]):
            assert view[1] + s["c"] <= view[0], s["name"]
    assert {s["kernel"] for s in fc.FIR_CASES} == set(fc.FIR_KERNELS)
    blur = of_kernel("blur4")
    # output heights shorter than a strip, every remainder of the strip height, widths 1, 2 and more
    assert {s["oh"] for s in blur} >= {1, 2, 3} and {s["oh"] % FIR_ROWS for s in blur if s["oh"] > FIR_ROWS} == {0, 1, 2, 3}
    assert {s["ih"] for s in blur} >= {1, 2, 3, 4, 5, 6, 13} and {s["iw"] for s in blur} >= {1, 2, 10}
    assert {s["pad0"] for s in blur} >= {(2, 2), (1, 1), (2, 1), (0, 3), (-1, 0)}
    # a strip whose input rows end past ih; one whose output rows end past oh
    assert any(-(-s["oh"] // FIR_ROWS) * FIR_ROWS + 3 - s["pad0"][0] > s["ih"] for s in blur)
    assert {(s["x"], s["y"]) for s in blur} == {((8, 0), (8, 0)), fc.SLICES}
    assert {(s["ih"], s["iw"]) for s in of_kernel("up2")} == {(5, 7), (1, 1)}
    assert {s["pad0"] for s in of_kernel("up2")} == {(2, 2), (1, 2)}
    assert all((s["oh"], s["ow"]) == (2 * s["ih"], 2 * s["iw"]) for s in of_kernel("up2") if s["pad0"] == (2, 2))
    assert {(s["ih"], s["iw"]) for s in of_kernel("down2")} == {(10, 10), (9, 7)}
    assert {s["pad0"] for s in of_kernel("down2")} == {(1, 1), (2, 0)}
    gen = of_kernel("generic")
    assert {(s["kh"], s["kw"]) for s in gen} >= {(3, 3), (1, 4), (4, 1), (5, 2), (8, 8)}
    assert {(s["up"], s["down"]) for s in gen} >= {(3, 1), (2, 2), (2, 3)}
    assert any((s["kh"], s["kw"], s["up"], s["down"]) == (4, 4, 2, 2) for s in gen)
    sc = of_kernel("scalar")
    forms = {(4, 4, 1, 1), (4, 4, 2, 1), (4, 4, 1, 2), (5, 2, 3, 2)}
    for pred in (lambda s: s["c"] == 3, lambda s: s["c"] == 8 and s["x"] == (12, 2), lambda s: s["c"] == 8 and s["y"] == (9, 1),
                 lambda s: s["c"] == 8 and s["bias"] == "offset" and fc.aligned(s["x"]) and fc.aligned(s["y"])):
        assert {(s["kh"], s["kw"], s["up"], s["down"]) for s in sc if pred(s)} == forms
    # every kernel sees the four epilogues
    for kernel in fc.FIR_KERNELS:
        epi = {(s["bias"] is not None, s["gain"], s["act"]) for s in of_kernel(kernel)}
        assert epi == {(False, 1.0, fc.ACT_NONE), (True, 1.5, fc.ACT_NONE), (True, 1.5, fc.ACT_LRELU),
                       (True, 1.5, fc.ACT_RELU)}, kernel
    # asymmetric pads in most cases, negative ones in some; outputs larger than upfirdn2d's own
    rnd = [s for s in fc.FIR_CASES if s["values"] == "rand"]
    assert sum(s["pad0"][0] != s["pad0"][1] for s in rnd) > len(rnd) // 2
    assert sum(min(s["pad0"]) < 0 for s in rnd) >= 4
    tall = [s for s in rnd if (s["oh"] - 1) * s["down"] + s["kh"] > s["ih"] * s["up"] + s["pad0"][0] + s["kh"] - 1]
    assert {s["kernel"] for s in tall} >= {"blur4", "generic"}
    assert {s["kernel"] for s in fc.FIR_CASES if s["values"] == "exact"} == {"blur4", "up2", "down2", "scalar"}


def test_fir_inputs():
    for i, s in enumerate(fc.FIR_CASES):
        d = fc.fir_case(i)
        k = d["k"]
        assert d["ref64"].shape == (s["n"], s["oh"], s["ow"], s["c"]) == d["unit"].shape == d["fma32"].shape
        assert torch.isfinite(d["ref64"]).all()
        if s["values"] == "exact":
            assert torch.equal(k, fc.gpen_filter(s["up"])) and float(k.sum()) == s["up"] ** 2
            for t in (d["x"], d["bias"]):
                assert torch.equal(t * 8, torch.round(t * 8)) and float(t.abs().max()) <= 1.0
            assert (s["gain"], s["post"], s["act"]) == (1.0, 1.0, fc.ACT_NONE)
            # representable: the float32 evaluations are the float64 reference, whatever the order
            assert torch.equal(d["fma32"].double(), d["ref64"]) and torch.equal(d["conv32"].double(), d["ref64"])
        else:
            # asymmetric: neither flip nor the transpose gives the filter back
            if k.numel() > 1:
                assert not torch.equal(k, torch.flip(k, [0, 1]))
            if k.shape[0] == k.shape[1]:
                assert not torch.equal(k, k.t())
        if s["bias"] is not None:
            assert torch.equal(d["bias"], d["bias_full"][1:1 + s["c"]])


def test_fir_reference_is_upfirdn2d():
    """Wherever a case's output is upfirdn2d's own for some pad (p0, p1) on both axes, the reference without
    its epilogue is oracle.enhancers.upfirdn2d in float64."""
    from oracle.enhancers import upfirdn2d
    agreed = set()
    for i, s in enumerate(fc.FIR_CASES):
        (py0, px0), up, down = s["pad0"], s["up"], s["down"]
        p1y = (s["oh"] - 1) * down + s["kh"] - s["ih"] * up - py0
        p1x = (s["ow"] - 1) * down + s["kw"] - s["iw"] * up - px0
        if py0 != px0 or p1y != p1x:
            continue
        d = fc.fir_case(i)
        x = d["x"].permute(0, 3, 1, 2).double()
        want = upfirdn2d(x, d["k"].double(), up=up, down=down, pad=(py0, p1y))
        got = fc.upfirdn_ref(x, d["k"].double(), up, down, py0, px0, s["oh"], s["ow"])
        assert want.shape == got.shape, s["name"]
        assert float((want - got).abs().max()) <= 1e-13, s["name"]
        agreed.add((s["kernel"], up, down))
    assert agreed >= {("blur4", 1, 1), ("up2", 2, 1), ("down2", 1, 2), ("generic", 1, 1)}, agreed
    for i, case in enumerate(fc.PLANE_CASES):
        _, _, up, down, pad, h, w = case
        d = fc.plane_case(i)
        want = upfirdn2d(d["x"].double(), d["k"].double(), up=up, down=down, pad=pad)
        assert want.shape == d["ref64"].shape and float((want - d["ref64"]).abs().max()) <= 1e-13, case[0]


def plane_kernel(case) -> str:
    """upfirdn2d_t's choice for a [N * C, H, W, 1] call with a 4x4 filter."""
    _, _, up, down, (p0, _), _, _ = case
    return "plane4" if p0 >= 0 and ((up == 1 and down <= 2) or (up == 2 and down == 1)) else "generic"


def test_plane_cases_straddle_the_tile():
    assert (PLANE_TY, PLANE_TX) == (16, 64)
    sizes = {}
    for case in fc.PLANE_CASES:
        assert plane_kernel(case) == case[1], case[0]
        assert case[4][0] != case[4][1], "asymmetric pads"
        sizes.setdefault((case[1], case[2], case[3]), set()).add(fc.plane_out_hw(case))
    for form in ((1, 1), (2, 1), (1, 2)):
        got = sizes[("plane4",) + form]
        assert {h for h, _ in got} == {PLANE_TY, PLANE_TY + 1} and {w for _, w in got} == {PLANE_TX, PLANE_TX + 1}, form
        assert ("generic",) + form in sizes, "a negative pad of the same form"


# ----------------------------------------------------------------------------- FFT: dispatch
def lds_floats(h, w, inverse):
    """The dynamic LDS of the generic kernels with 4 channels per block (s2v_rfft2 / s2v_irfft2)."""
    wf = w // 2 + 1
    if inverse:
        return 4 * (h * wf * 4) + 2 * h * h + 2 * w * wf
    return 4 * (h * w + h * wf * 2) + 2 * wf * w + 2 * h * h + 4 * h


def fft_kernel(s, inverse) -> str:
    assert s["c"] % 4 == 0 and s["w"] > 1 and s["scs"] >= 2 * s["c"] and s["scs"] % 4 == 0
    if not inverse:
        assert fc.aligned(s["x"]), "rfft2 refuses a misaligned x"
    assert lds_floats(s["h"], s["w"], inverse) * 4 <= FFT_LDS_KB * 1024, "the tile fits"
    return "mfma" if s["h"] == s["w"] and s["h"] in FFT_MF_SIZES else "generic"


def test_fft_cases_reach_their_kernels():
    assert FFT_MF_SIZES == (12, 24, 48) and FFT_LDS_KB == 160
    by = {s["name"]: s for s in fc.FFT_CASES}
    assert len(by) == len(fc.FFT_CASES)
    for s in fc.FFT_CASES:
        for inverse in (False, True):
            assert fft_kernel(s, inverse) == s["kernel"], s["name"]
        assert s["n"] * s["c"] <= s["h"] * s["w"], "an impulse position for every (image, channel)"
    mf = [(s["h"], s["n"], s["c"]) for s in fc.FFT_CASES if s["kernel"] == "mfma"]
    assert set(mf) == {(12, 3, 8), (12, 8, 4), (12, 8, 12), (12, 16, 8), (24, 3, 8), (24, 8, 8), (48, 1, 4), (48, 8, 8)}
    # the XCD permutation is a permutation, and it differs from the plain order with 2 and 3 groups per image
    for h, n, c in mf:
        order = fc.xcd_order(n, c // 4)
        assert sorted(order) == [(i, g) for i in range(n) for g in range(c // 4)]
        plain = [(b // (c // 4), b % (c // 4)) for b in range(n * (c // 4))]
        assert (order != plain) == (n % 8 == 0 and c > 4), (h, n, c)
    assert {c // 4 for _, n, c in mf if n % 8 == 0} == {1, 2, 3}
    gen = {(s["h"], s["w"]) for s in fc.FFT_CASES if s["kernel"] == "generic"}
    assert gen == {(6, 10), (5, 7), (13, 13), (1, 8), (7, 2), (24, 12), (40, 56), (56, 56)}
    for name, kb in (("g40x56", 100), ("g56x56", 142)):
        s = by[name]
        sizes = [lds_floats(s["h"], s["w"], inv) * 4 for inv in (False, True)]
        assert all(64 * 1024 < b <= FFT_LDS_KB * 1024 for b in sizes) and abs(max(sizes) / 1000 - kb) < 1, (name, sizes)
        assert (s["n"], s["c"]) == (1, 4)
    assert lds_floats(6, 10, False) * 4 < 64 * 1024
    assert all(lds_floats(64, 64, inv) * 4 > FFT_LDS_KB * 1024 for inv in (False, True)), "64x64 is a rejection"
    assert (by["g13x13-c8"]["n"], by["g13x13-c8"]["c"]) == (2, 8)
    # every view form on both kernel families
    for kernel in ("mfma", "generic"):
        cs = [s for s in fc.FFT_CASES if s["kernel"] == kernel]
        assert {s["x"][1] for s in cs} == {0, 4}
        assert {s["scs"] - 2 * s["c"] for s in cs} == {0, 8}
        assert {None if s["res"] is None else s["res"][1] for s in cs} == {None, 0, 2}
        assert {s["y"][1] for s in cs} == {0, 1}
        assert all(s["res"] is None or s["res"] in ((s["c"], 0), (s["c"] + 5, 2)) for s in cs)
        assert all(s["y"] in ((s["c"], 0), (s["c"] + 3, 1)) for s in cs)


def test_fft_value_sets():
    for i, s in enumerate(fc.FFT_CASES):
        n, c, h, w = s["n"], s["c"], s["h"], s["w"]
        f = h * (w // 2 + 1)
        d = fc.fft_case(i, "impulse")
        for t, slots in ((d["x"].reshape(n, h * w, c), h * w), (d["sp"].reshape(n, f, 2, c).reshape(n, 2 * f, c), 2 * f)):
            nz = t != 0
            assert (nz.sum(1) == 1).all(), "one sample per (image, channel)"
            pos = nz.float().argmax(1).flatten()
            amp = t.sum(1).flatten()
            assert len(set(pos.tolist())) == n * c and len(set(amp.tolist())) == n * c, s["name"]
        d = fc.fft_case(i, "offset")
        if h * w >= 16:
            spec = d["spec64"].abs()
            rest = spec.clone()
            rest[:, 0, :c] = 0
            assert (spec[:, 0, :c].amin() > 8 * rest.amax()), s["name"]          # the DC bin dominates


# ----------------------------------------------------------------------------- the references
def test_fft_reference_is_torch_fft():
    """The float64 passes with the float32 tables lie within ffc_cases' transform rule of torch.fft.rfftn /
    irfftn(s=(h, w)), norm="ortho", in float64: also for the inverse of spectra that are not
    Hermitian-consistent, whose imaginary parts at DC and Nyquist torch's c2r ignores."""
    for i, v in fc.FFT_RUNS:
        s, d = fc.FFT_CASES[i], fc.fft_case(i, v)
        n, c, h, w = s["n"], s["c"], s["h"], s["w"]
        z = torch.fft.rfftn(d["x"].double(), dim=(1, 2), norm="ortho")
        want = fc.to_spec(z.real, z.imag)
        tol, e_ref, _ = fc.transform_tol(want, d["spec_mm32"])
        err = float((d["spec64"] - want).abs().max())
        assert err <= tol, (fc.FFT_IDS[fc.FFT_RUNS.index((i, v))], "forward", err, tol)
        zr, zi = fc.from_spec(d["sp"].double(), h)
        want = torch.fft.irfftn(torch.complex(zr, zi), s=(h, w), dim=(1, 2), norm="ortho")
        if d["res"] is not None:
            want = want + d["res"].double()
        tol, e_ref, _ = fc.transform_tol(want, d["y_mm32"])
        err = float((d["y64"] - want).abs().max())
        assert err <= tol, (fc.FFT_IDS[fc.FFT_RUNS.index((i, v))], "inverse", err, tol)
        if v == "unit":
            # the spectrum is not Hermitian-consistent: its DC (and Nyquist) column has imaginary parts that
            # the H pass mixes into the real part of that column
            assert float(zi[:, :, 0].abs().max()) > 0.5


# ----------------------------------------------------------------------------- the bound constants
def ratio(got, ref64, bound) -> float:
    return float(((got.double() - ref64).abs() / bound).max())


def test_fir_bound_constant_is_the_smallest_power_of_two():
    """Both float32 evaluations stay within half the bound on every FIR and plane case with K_FIR, and not with
    K_FIR / 2."""
    worst = {"conv32": (0.0, ""), "fma32": (0.0, "")}
    runs = [(s["name"], fc.fir_case(i)) for i, s in enumerate(fc.FIR_CASES)]
    runs += [("plane " + c[0], fc.plane_case(i)) for i, c in enumerate(fc.PLANE_CASES)]
    for name, d in runs:
        b = fc.fir_bound(d)
        assert d["unit"].shape == d["ref64"].shape and (d["unit"] >= 0).all()
        r = {k: ratio(d[k], d["ref64"], b) for k in worst}
        print(f"fir {name}: K={fc.K_FIR} float32 err / bound: conv2d form {r['conv32']:.3f}, fma chain {r['fma32']:.3f}")
        for k in worst:
            assert r[k] <= 0.5, (name, k, r[k])
            worst[k] = max(worst[k], (r[k], name))
    print(f"worst: {worst}")
    k = fc.K_FIR
    assert k & (k - 1) == 0 and max(v[0] for v in worst.values()) > 0.25, "K / 2 would do"


def test_fft_bound_constant_is_the_smallest_power_of_two():
    worst = {}
    for i, v in fc.FFT_RUNS:
        d = fc.fft_case(i, v)
        name = fc.FFT_IDS[fc.FFT_RUNS.index((i, v))]
        line = f"fft {name}: K={fc.K_FFT} float32 err / bound:"
        for direction, ref, unit, pre in (("forward", "spec64", "spec_unit", "spec"), ("inverse", "y64", "y_unit", "y")):
            b = fc.fft_bound(d[unit])
            assert d[unit].shape == d[ref].shape and torch.isfinite(d[ref]).all()
            for form in ("mm32", "fma32"):
                r = ratio(d[f"{pre}_{form}"], d[ref], b)
                line += f" {direction} {form} {r:.3f}"
                assert r <= 0.5, (name, direction, form, r)
                worst[(direction, form)] = max(worst.get((direction, form), (0.0, "")), (r, name))
        print(line)
    print(f"worst: {worst}")
    k = fc.K_FFT
    assert k & (k - 1) == 0 and max(v[0] for v in worst.values()) > 0.25, "K / 2 would do"


# ----------------------------------------------------------------------------- wrong variants
def test_fir_bound_catches_wrong_kernels():
    """An unflipped filter, py0 / px0 swapped, the zero-insertion test dropped (up read as dense) and a strip
    kernel that gives every row of a strip row 0's taps: each exceeds the bound on a case of its table."""
    best = {}
    for i, s in enumerate(fc.FIR_CASES):
        d = fc.fir_case(i)
        x, k = d["x"].permute(0, 3, 1, 2).double(), d["k"].double()
        (py0, px0), up, down, oh, ow = s["pad0"], s["up"], s["down"], s["oh"], s["ow"]

        def finish(fir):
            b = d["bias"].double()[None, :, None, None] if d["bias"] is not None else 0.0
            out = fc.f32(s["post"]) * fc.act_ref(fc.f32(s["gain"]) * fir + b, s["act"], fc.f32(s["alpha"]))
            return float(((out.permute(0, 2, 3, 1) - d["ref64"]).abs() / fc.fir_bound(d)).max())

        right = fc.upfirdn_ref(x, k, up, down, py0, px0, oh, ow)
        assert finish(right) == 0.0
        muts = {"unflipped filter": fc.upfirdn_ref(x, k, up, down, py0, px0, oh, ow, flip=False)}
        if py0 != px0:
            muts["pads swapped"] = fc.upfirdn_ref(x, k, up, down, px0, py0, oh, ow)
        if up > 1:
            muts["no zero insertion"] = fc.upfirdn_ref(x, k, up, down, py0, px0, oh, ow, insert_zeros=False)
        if s["kernel"] == "blur4" and oh > 1:
            rows = torch.arange(oh) // FIR_ROWS * FIR_ROWS
            muts["row 0's taps in every strip row"] = right[:, :, rows]
        for name, wrong in muts.items():
            r = finish(wrong)
            print(f"fir {s['name']}: {name}: err / bound = {r:.3g}")
            key = (s["kernel"], name)
            best[key] = max(best.get(key, 0.0), r)
    for kernel in fc.FIR_KERNELS:
        assert best[(kernel, "unflipped filter")] >= 100.0 and best[(kernel, "pads swapped")] >= 100.0, kernel
    for kernel in ("up2", "generic", "scalar"):
        assert best[(kernel, "no zero insertion")] >= 100.0, kernel
    assert best[("blur4", "row 0's taps in every strip row")] >= 100.0
    # the symmetric GPEN filter of the exact set (and of the earlier test) cannot see the flip
    i = fc.FIR_IDS.index(next(s["name"] for s in fc.FIR_CASES if s["values"] == "exact"))
    d, s = fc.fir_case(i), fc.FIR_CASES[i]
    x = d["x"].permute(0, 3, 1, 2).double()
    args = (s["up"], s["down"], *s["pad0"], s["oh"], s["ow"])
    assert torch.equal(fc.upfirdn_ref(x, d["k"].double(), *args), fc.upfirdn_ref(x, d["k"].double(), *args, flip=False))


def test_fft_bound_catches_wrong_kernels():
    """+fi for -fi in the forward H pass; the imaginary half stored at scs / 2 instead of C; the XCD order
    applied to the stores but not the loads (image and channel group swapped); a c2r pass that gives the
    imaginary parts of the DC and Nyquist columns the real parts' weights instead of ignoring them."""
    best = {}

    def note(name, r, what):
        print(f"fft {what}: {name}: err / bound = {r:.3g}")
        best[name] = max(best.get(name, 0.0), r)

    for i, v in fc.FFT_RUNS:
        s, d = fc.FFT_CASES[i], fc.fft_case(i, v)
        n, c, h, w, scs = s["n"], s["c"], s["h"], s["w"], s["scs"]
        what = fc.FFT_IDS[fc.FFT_RUNS.index((i, v))]
        fb, ib = fc.fft_bound(d["spec_unit"]), fc.fft_bound(d["y_unit"])
        if h > 2:
            note("H-pass sign", ratio(fc.rfft_passes(d["x"], h_sign=1.0), d["spec64"], fb), what)
        if scs > 2 * c:
            full = torch.zeros(n, d["spec64"].shape[1], scs, dtype=torch.float64)
            full[..., :c] = d["spec64"][..., :c]
            full[..., scs // 2:scs // 2 + c] = d["spec64"][..., c:]
            note("imaginary half at scs / 2", ratio(full[..., :2 * c], d["spec64"], fb), what)
        groups = c // 4
        if s["kernel"] == "mfma" and n % 8 == 0 and groups > 1:
            for ref, bound, key in ((d["spec64"], fb, "forward"), (d["y64"], ib, "inverse")):
                wrong = ref.clone()
                last = ref.shape[-1]
                for b, (img, g) in enumerate(fc.xcd_order(n, groups)):
                    src_img, src_g = b // groups, b % groups
                    for part in range(last // c):
                        lo = part * c
                        wrong[img, ..., lo + 4 * g:lo + 4 * g + 4] = ref[src_img, ..., lo + 4 * src_g:lo + 4 * src_g + 4]
                note("image and group swapped", ratio(wrong, ref, bound), f"{what} {key}")
        _, _, _, iw = fc.tables(h, w)
        iw = iw.clone()
        iw[0, 1] = iw[0, 0]
        if w % 2 == 0:
            iw[w // 2, 1] = iw[w // 2, 0]
        note("DC / Nyquist imaginary part not ignored", ratio(fc.irfft_passes(d["sp"], h, w, d["res"], iw=iw), d["y64"], ib), what)
    for name in ("H-pass sign", "imaginary half at scs / 2", "image and group swapped",
                 "DC / Nyquist imaginary part not ignored"):
        assert best[name] >= 100.0, (name, best[name])
