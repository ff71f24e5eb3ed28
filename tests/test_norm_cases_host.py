"""CPU checks of the tables that tests/test_norm_direct_gpu.py feeds the norm, resize, pad and row-pack
kernels (tests/norm_cases.py): every case reaches the path it is listed for (the launch arithmetic is
recomputed here from the constants in csrc/norm.hip and csrc/misc.hip), the bound constant K is the smallest
that two CPU float32 evaluations keep, the resize reference agrees with F.interpolate, and a deliberately
wrong variant of every kernel family lands far outside the tolerance.  Run with ``-s`` for the figures."""
import os
import re

import torch
import torch.nn.functional as F

import norm_cases as nc
import s2v_import

CSRC = os.path.join(s2v_import.PKG_DIR, "csrc")


def source(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def grab(text, pattern):
    m = re.search(pattern, text)
    assert m, f"the launch arithmetic changed: {pattern!r} is no longer in the source"
    return [int(g) for g in m.groups()]


# ----------------------------------------------------------------------------- launch arithmetic
NORM = source("norm.hip")
MISC = source("misc.hip")
(LN_ROUND, LN_PER), (LN_MAXBLK,) = grab(NORM, r"b = \(elems \+ (\d+)\) / (\d+);"), grab(NORM, r"if \(b > (\d+)\) b = \1;")
(LN_EPT,) = grab(NORM, r"constexpr int LN_EPT = (\d+);")
LN_CAP_N, LN_CAP, LN_CAP_TOTAL = grab(NORM, r"cap = n >= (\d+) \? (\d+) : (\d+) / n;")
(IN_QB_MAX,) = grab(NORM, r"int in_quads\(int c\) \{ return c / 4 < (\d+) \?")
(ROWS_MAX,) = grab(MISC, r"rows < (\d+) \? rows : \1")
(ROWS_PER_BLOCK,) = grab(MISC, r"gy = \(rows \+ \d+\) / (\d+);")


def ln_blocks(elems):
    assert LN_ROUND == LN_PER - 1
    return max(1, min(LN_MAXBLK, (elems + LN_ROUND) // LN_PER))


def ln_stats_path(s):
    c, (xcs, xoff) = s["c"], s["x"]
    if c % 4 == 0 and xoff % 4 == 0 and xcs == c:
        return "dense4"
    if c % 4 == 0 and xoff % 4 == 0 and xcs % 4 == 0:
        return "strided4"
    return "scalar"


def ln_apply_path(s):
    return "vec" if s["c"] % 4 == 0 and all(nc.aligned(s[k]) for k in ("x", "y", "res")) else "scalar"


def test_layernorm_cases_reach_their_paths():
    by = {s["name"]: s for s in nc.LN_CASES}
    assert len(by) == len(nc.LN_CASES)
    for s in nc.LN_CASES:
        assert ln_stats_path(s) == s["stats"] and ln_apply_path(s) == s["apply"], s["name"]
        assert s["x"][1] + s["c"] <= s["x"][0] and s["y"][1] + s["c"] <= s["y"][0]
    for name in ("cap64", "cap64-odd"):
        s = by[name]
        hw, c4 = s["h"] * s["w"], s["c"] // 4
        nblk = ln_blocks(hw * s["c"])
        per = -(-hw // nblk)
        # the four-loads-in-flight loop (e + 768 < tot) runs in the statistics blocks
        assert nblk > 1 and per * c4 > 768 + 255
        quads = hw * c4
        uncapped = -(-quads // (256 * LN_EPT))
        cap = LN_CAP if s["n"] >= LN_CAP_N else LN_CAP_TOTAL // s["n"]
        assert cap < uncapped <= 2 * cap, (name, cap, uncapped)       # some blocks loop twice, some once
        assert s["pools"] == (False, True)
        print(f"layernorm2d {name}: {nblk} stats blocks of {per} pixels, apply grid {cap} of {uncapped} blocks, "
              f"{quads - cap * 256 * LN_EPT} quads in the second step")
    assert (by["cap64-odd"]["h"] * by["cap64-odd"]["w"] * 16) % (256 * LN_EPT), "a ragged last step"
    assert by["cap64-odd"]["h"] % 2 and by["cap64-odd"]["w"] % 2
    s = by["odd-slice"]
    assert s["h"] % 2 and s["w"] % 2 and (s["h"] // 2, s["w"] // 2) == (3, 2) and s["y"][0] > s["c"]
    s = by["misaligned"]
    assert s["c"] % 4 == 0 and s["x"][1] % 4 and s["x"][0] % 4 == 0
    s = by["empty-blocks"]
    hw, nblk = s["h"] * s["w"], ln_blocks(s["h"] * s["w"] * s["c"])
    per = -(-hw // nblk)
    assert nblk == 6 and hw == 3 and sum(b * per >= hw for b in range(nblk)) == 3
    s = by["small"]
    assert s["h"] * s["w"] * s["c"] <= 256 and s["c"] == 4
    # acts, residual and eps settings across the list
    assert {s["act"] for s in nc.LN_CASES} == {nc.ACT_NONE, nc.ACT_RELU, nc.ACT_LRELU}
    assert {s["res"] is None for s in nc.LN_CASES} == {False, True}
    assert {s["eps"] for s in nc.LN_CASES} == {1e-5, 1e-3}
    d = nc.ln_case([s["name"] for s in nc.LN_CASES].index("offset"), False)
    spread = 1.0 / d["rstd"]
    assert (d["mean"].abs() > 50 * spread).all()


def in_quads(c):
    return min(c // 4, IN_QB_MAX)


def in_fused_qb(n, c):
    qb = in_quads(c)
    while qb > 4 and n * -(-c // (4 * qb)) < 512:
        qb //= 2
    return qb


def test_instnorm_cases_reach_their_paths():
    names = [s["name"] for s in nc.IN_CASES]
    assert len(set(names)) == len(names)
    vec = [s for s in nc.IN_CASES if s["path"] == "vector"]
    for s in nc.IN_CASES:
        is_vec = s["c"] % 4 == 0 and all(nc.aligned(s[k]) for k in ("x", "y", "res", "pad"))
        assert is_vec == (s["path"] == "vector"), s["name"]
        assert (s["pad"] is not None) == (is_vec and s["h"] >= 2 and s["w"] >= 2), s["name"]
        if s["pad"] is not None:
            assert s["pad"] == (s["c"] + 8, 4)
    assert {in_quads(s["c"]) for s in vec} >= {1, 10, 64}
    # 250 live threads of 256; a second channel block with one live quad (both forms)
    assert 256 // in_quads(40) * in_quads(40) == 250
    assert 260 // 4 - in_quads(260) == 1 and (260 // 4) % in_fused_qb(3, 260) == 1
    assert any(s["c"] % 4 for s in nc.IN_CASES), "scalar by channel count"
    assert any(s["c"] % 4 == 0 and s["x"][1] % 4 for s in nc.IN_CASES), "scalar by misalignment"
    forms = {f for _, f in nc.IN_RUNS}
    assert forms == {"fused", "two"}
    for s in vec:
        assert ("fused" in nc.in_forms(s)) == (s["h"] * s["w"] <= 1023)
    assert any("fused" not in nc.in_forms(s) for s in vec)
    for c in (4, 40, 260):
        planes = {(s["h"], s["w"]) for s in vec if s["c"] == c}
        assert planes == set(nc.IN_PLANES), c
    # what a plane with 3 rows / 3 columns needs is reached in both forms, with the padded output
    for pred in (lambda s: s["h"] == 3, lambda s: s["w"] == 3, lambda s: s["h"] == 3 and s["w"] == 3,
                 lambda s: s["h"] == 2, lambda s: s["w"] == 2):
        hit = [s for s in vec if pred(s) and s["pad"] is not None]
        assert hit and all(nc.in_forms(s) == ("fused", "two") for s in hit)
    padded = [s for s in vec if s["pad"] is not None]
    for key, values in (("n", {1, 3}), ("gb", {False, True}), ("act", {nc.ACT_NONE, nc.ACT_RELU, nc.ACT_LRELU}),
                        ("eps", {1e-5, 1e-3})):
        assert {s[key] for s in padded} == values, key
    assert {s["n"] for s in nc.IN_CASES if s["path"] == "scalar"} == {1, 3}
    assert {s["res"] is None for s in padded} == {False, True}
    assert all(s["res"] is None or s["res"][0] > s["c"] for s in nc.IN_CASES), "res is a slice"
    off = [s for s in nc.IN_CASES if s["values"] == "offset"]
    assert [(s["h"], s["w"], s["c"]) for s in off] == [(12, 12, 32)]


# ----------------------------------------------------------------------------- the bound
def ratios(d, k=nc.K_BOUND):
    b = k * d["unit"] + nc.TINY
    return (float(((d["torch32"].double() - d["ref64"]).abs() / b).max()),
            float(((d["fma32"].double() - d["ref64"]).abs() / b).max()))


def test_norm_bound_constant_is_the_smallest_power_of_two():
    """Both float32 evaluations stay within half the bound on every case with the recorded K, and not with
    K / 2."""
    worst = [0.0, 0.0]
    runs = [(f"layernorm2d {nid}", nc.ln_case(i, p)) for nid, (i, p) in zip(nc.LN_IDS, nc.LN_RUNS)]
    runs += [(f"instnorm {s['name']}", nc.in_case(i)) for i, s in enumerate(nc.IN_CASES)]
    for what, d in runs:
        rt, rf = ratios(d)
        print(f"{what}: K={nc.K_BOUND} float32 err / bound: torch form {rt:.3f}, fma form {rf:.3f}")
        assert torch.isfinite(d["ref64"]).all() and d["ref64"].shape == d["torch32"].shape == d["unit"].shape
        assert rt <= 0.5 and rf <= 0.5, (what, rt, rf)
        worst = [max(worst[0], rt), max(worst[1], rf)]
    print(f"worst: torch form {worst[0]:.3f}, fma form {worst[1]:.3f}")
    k = nc.K_BOUND
    assert k & (k - 1) == 0 and max(worst) > 0.25, "K / 2 would do: K is not the smallest power of two"


def test_layernorm_reference_is_layer_norm():
    for (i, pool), nid in zip(nc.LN_RUNS, nc.LN_IDS):
        s, d = nc.LN_CASES[i], nc.ln_case(i, pool)
        x = d["x"].double()
        shape = x.shape[1:]
        ref = F.layer_norm(x, shape, d["weight"].double().expand(shape), d["bias"].double().expand(shape), nc.f32(s["eps"]))
        ref = nc.act_ref(ref, s["act"], nc.f32(s["alpha"]))
        if pool:
            ref = F.avg_pool2d(ref.permute(0, 3, 1, 2), 2).permute(0, 2, 3, 1)
        if d["res"] is not None:
            ref = ref + d["res"].double()
        err = float((ref - d["ref64"]).abs().max())
        assert err <= 1e-12 * max(1.0, float(ref.abs().max())), (nid, err)


def test_layernorm_const_is_exactly_act_bias_plus_res():
    i = [s["name"] for s in nc.LN_CASES].index("const")
    for pool in (False, True):
        d = nc.ln_case(i, pool)
        assert (d["x"] == 0.75).all() and d["res"] is not None
        want = F.relu(d["bias"]).double() + d["res"].double()
        assert torch.equal(d["ref64"], want)
        assert (F.relu(d["bias"]) == 0).any() and (F.relu(d["bias"]) > 0).any()


def test_instnorm_reference_is_instance_norm():
    for i, s in enumerate(nc.IN_CASES):
        d = nc.in_case(i)
        if s["h"] * s["w"] == 1:
            continue                        # F.instance_norm refuses one value per channel
        x = d["x"].double().permute(0, 3, 1, 2)
        ref = F.instance_norm(x, eps=nc.f32(s["eps"]))
        if s["gb"]:
            c = s["c"]
            assert d["gb"].shape[1] == 2 * c + 4 != c
            ref = ref * (1 + d["gb"][:, :c].double()[:, :, None, None]) + d["gb"][:, c + 4:].double()[:, :, None, None]
        ref = nc.act_ref(ref, s["act"], nc.f32(s["alpha"])).permute(0, 2, 3, 1)
        if d["res"] is not None:
            ref = ref + d["res"].double()
        # a cross-check of the formula only: F.instance_norm on the CPU agrees with the plain fp64 formula to
        # about 2^-25 relative (4.5e-8 at c4-2x2), no closer, also for float64 input
        err = float((ref - d["ref64"]).abs().max())
        assert err <= 2e-7 * max(1.0, float(ref.abs().max())), (s["name"], err)


# ----------------------------------------------------------------------------- wrong variants
def mutant_ratio(d, wrong64):
    return float(((wrong64 - d["ref64"]).abs() / nc.bound_of(d)).max())


def _affine(x64, mean, var, eps, scale, shift, s, res, after_sqrt=False):
    rstd = 1.0 / (torch.sqrt(var) + eps) if after_sqrt else 1.0 / torch.sqrt(var + eps)
    v = nc.act_ref((x64 - mean) * rstd * scale.double() + shift.double(), s["act"], nc.f32(s["alpha"]))
    return v if res is None else v + res.double()


def norm_mutants(x, dims, wrong_dims, eps, scale, shift, s, res):
    x64 = x.double()
    mean = x64.mean(dim=dims, keepdim=True)
    var = ((x64 - mean) ** 2).mean(dim=dims, keepdim=True)
    cnt = 1
    for a in dims:
        cnt *= x.shape[a]
    wmean = x64.mean(dim=wrong_dims, keepdim=True)
    wvar = ((x64 - wmean) ** 2).mean(dim=wrong_dims, keepdim=True)
    out = {"eps after the root": _affine(x64, mean, var, eps, scale, shift, s, res, after_sqrt=True),
           "wrong axis set": _affine(x64, wmean, wvar, eps, scale, shift, s, res)}
    if cnt > 1:
        out["unbiased variance"] = _affine(x64, mean, var * cnt / (cnt - 1), eps, scale, shift, s, res)
    return out, cnt


def test_norm_bounds_catch_wrong_statistics():
    """Unbiased variance, eps added after the square root, moments over the wrong axes: each exceeds the bound
    at least 10 times on a case of at most 256 reduced elements (at 270336 elements the unbiased variance is
    within the bound, which is why the small cases are in the list)."""
    best = {}
    for i, s in enumerate(nc.LN_CASES):
        if s["values"] == "const":
            continue
        d = nc.ln_case(i, False)
        muts, cnt = norm_mutants(d["x"], (1, 2, 3), (1, 2), nc.f32(s["eps"]), d["weight"], d["bias"], s, d["res"])
        for name, wrong in muts.items():
            r = mutant_ratio(d, wrong)
            print(f"layernorm2d {s['name']} ({cnt} reduced): {name}: err / bound = {r:.3g}")
            if cnt <= 256:
                best[("ln", name)] = max(best.get(("ln", name), 0.0), r)
    for i, s in enumerate(nc.IN_CASES):
        d = nc.in_case(i)
        c = s["c"]
        scale = 1.0 + d["gb"][:, None, None, :c] if s["gb"] else torch.ones(1, 1, 1, c)
        shift = d["gb"][:, None, None, c + 4:] if s["gb"] else torch.zeros(1, 1, 1, c)
        muts, cnt = norm_mutants(d["x"], (1, 2), (1, 2, 3), nc.f32(s["eps"]), scale, shift, s, d["res"])
        for name, wrong in muts.items():
            r = mutant_ratio(d, wrong)
            print(f"instnorm {s['name']} ({cnt} reduced): {name}: err / bound = {r:.3g}")
            if cnt <= 256:
                best[("in", name)] = max(best.get(("in", name), 0.0), r)
    for fam in ("ln", "in"):
        for name in ("unbiased variance", "eps after the root", "wrong axis set"):
            assert best[(fam, name)] >= 10.0, (fam, name, best[(fam, name)])


def align_corners_taps(scale, in_size, out_size):
    dst = torch.arange(out_size, dtype=torch.float32)
    src = dst * (float(in_size - 1) / max(out_size - 1, 1))
    i0 = src.to(torch.int64)
    i1 = i0 + (i0 < in_size - 1).long()
    l1 = src - i0.float()
    return i0, i1, 1.0 - l1, l1, src


def test_resize_reference_and_cases():
    """ref64's float32 taps are F.interpolate's (e_ref <= 8 * 2^-24 * max|x|); every bilinear case reaches
    the first and the last source line on both axes, and every axis that is upsampled has outputs whose
    coordinate clamps at 0 and outputs whose second tap clamps at in - 1 (a downsampled axis has neither:
    its first coordinate is positive and its last pair ends at in - 1 at the most); a shifted tap and
    align_corners=True coordinates are >= 10 tolerances away."""
    kernels = {}
    caught = {"tap shifted by one": 0.0, "align_corners=True": 0.0}
    for i, case in enumerate(nc.RESIZE_CASES):
        name, kernel, n, c, ih, iw = case[:6]
        d = nc.resize_case(i, 0)
        assert d["e_ref"] <= 8 * nc.EPS24 * float(d["x"].abs().max()), (name, d["e_ref"])
        up_clamped = []
        for scale, isz, osz in ((d["sh"], ih, d["oh"]), (d["sw"], iw, d["ow"])):
            i0, i1, l0, l1, raw = nc.bilinear_taps(scale, isz, osz)
            assert int(i0.min()) == 0 and int(i1.max()) == isz - 1, name
            assert (l0 >= 0).all() and (l1 >= 0).all() and int(i1.max()) < isz
            if osz > isz:
                assert (raw < 0).any() and ((i1 == i0) & (i0 == isz - 1)).any(), name
                up_clamped.append(True)
        kernels.setdefault(kernel, []).append(len(up_clamped))
        line = f"resize {name}: e_ref={d['e_ref']:.2e} floor={d['floor']:.2e} tol={d['tol']:.2e}"
        if ih > 1 and iw > 1 and (d["oh"], d["ow"]) != (ih, iw):
            shifted = nc.bilinear_ref64(d["x"], d["oh"], d["ow"], d["sh"], d["sw"], shift=1)
            ac = nc.bilinear_ref64(d["x"], d["oh"], d["ow"], d["sh"], d["sw"], coords=align_corners_taps)
            chk = F.interpolate(d["x"].double(), size=(d["oh"], d["ow"]), mode="bilinear", align_corners=True)
            assert float((ac - chk).abs().max()) < 1e-5
            for what, wrong in (("tap shifted by one", shifted), ("align_corners=True", ac)):
                r = float((wrong - d["ref64"]).abs().max()) / d["tol"]
                caught[what] = max(caught[what], r)
                line += f" {what}: {r:.3g} tol"
                assert r >= 10.0, (name, what, r)
        print(line)
    assert all(max(v) == 2 for v in kernels.values()), kernels       # both axes clamped in each kernel
    assert set(kernels) == {"generic", "float4", "x2"}
    assert min(caught.values()) >= 10.0


def test_resize_nearest_cases():
    """The float32 index rule min(floor(dst * scale), in - 1) with the scales ops.resize passes reproduces
    F.interpolate(mode='nearest'); the list has non-integer ratios; rounding instead of floor differs."""
    fractional = wrong = 0
    for i, case in enumerate(nc.RESIZE_CASES):
        name, _, n, c, ih, iw = case[:6]
        if 1 not in case[8]:
            continue
        d = nc.resize_case(i, 1)
        iy, ix = nc.nearest_index(d["sh"], ih, d["oh"]), nc.nearest_index(d["sw"], iw, d["ow"])
        assert torch.equal(d["x"][:, :, iy][:, :, :, ix], d["exact"]), name
        fractional += any(a % b and b % a for a, b in ((ih, d["oh"]), (iw, d["ow"])))
        ry = torch.round(torch.arange(d["oh"], dtype=torch.float32) * d["sh"]).long().clamp(max=ih - 1)
        rx = torch.round(torch.arange(d["ow"], dtype=torch.float32) * d["sw"]).long().clamp(max=iw - 1)
        differs = not torch.equal(d["x"][:, :, ry][:, :, :, rx], d["exact"])
        wrong += differs
        print(f"resize {name} nearest: rounding instead of floor {'differs' if differs else 'is the same'}")
    assert fractional >= 2 and wrong >= 2


def test_resize_row_loops_and_kernels():
    by = {c[0]: c for c in nc.RESIZE_CASES}
    n, ih = by["x2-rows"][2], by["x2-rows"][4]
    assert n * ih > ROWS_MAX and nc.resize_out_hw(by["x2-rows"]) == (2 * ih, 2)
    c = by["float4-rows"]
    oh, ow = nc.resize_out_hw(c)
    assert (c[2] * oh + ROWS_PER_BLOCK - 1) // ROWS_PER_BLOCK > ROWS_MAX and (oh, ow) == (2 * c[4], 2 * c[5])
    for name, kernel, n, c_, ih, iw, size, sf, modes in nc.RESIZE_CASES:
        oh, ow = nc.resize_out_hw(by[name])
        x2 = (oh, ow) == (2 * ih, 2 * iw) and c_ % 4 == 0
        assert (kernel == "x2") == x2, name
        assert (kernel == "generic") == (c_ % 4 != 0), name
        assert n * c_ * max(ih * iw, oh * ow) * 4 <= 9 << 20, "a few MB at the most"
    assert {c[3] for c in nc.RESIZE_CASES if c[1] == "x2"} >= {64, 32}


def test_pad_reflect_cases():
    """The pads are the asymmetric, the largest legal, the empty and the FFC's; a 'reflect' that repeats the
    edge pixel differs from the reference for every pad but the empty one."""
    n, h, w = nc.PAD_NHW
    assert nc.PAD_PADS == ((0, 3, 2, 0), (h - 1, 0, 0, w - 1), (0, 0, 0, 0), (1, 1, 1, 1))
    for name, c, xv, yv, kernel in nc.PAD_LAYOUTS:
        vec = c % 4 == 0 and nc.aligned(xv) and nc.aligned(yv)
        assert vec == (kernel == "float4"), name
    assert any(k == "float4" and yv[0] > c and xv[0] > c for _, c, xv, yv, k in nc.PAD_LAYOUTS)
    assert any(k == "scalar" and c % 4 == 0 for _, c, _, _, k in nc.PAD_LAYOUTS)
    for li, pi in nc.PAD_RUNS:
        d = nc.pad_case(li, pi)
        pt, pb, pl, pr = nc.PAD_PADS[pi]
        # numpy's 'symmetric' (the edge pixel repeated, then mirrored) by index
        iy = torch.tensor([(-1 - i) if i < 0 else (2 * h - 1 - i if i >= h else i) for i in range(-pt, h + pb)])
        ix = torch.tensor([(-1 - i) if i < 0 else (2 * w - 1 - i if i >= w else i) for i in range(-pl, w + pr)])
        edge = d["x"][:, iy][:, :, ix]
        assert edge.shape == d["exact"].shape
        differs = not torch.equal(edge, d["exact"])
        assert differs == (pt + pb + pl + pr > 0), nc.PAD_IDS[nc.PAD_RUNS.index((li, pi))]
    print("pad_reflect: the edge-repeating reflect differs on every padded case")


def test_row_pack_cases():
    """The reference writes +0.0 outside the row and past kw * c; pw off by one differs on every case."""
    for i, (name, n, h, w, c, kw, pw, ycs, xv) in enumerate(nc.PACK_CASES):
        d = nc.pack_case(i)
        assert ycs % 4 == 0 and ycs >= kw * c and xv[1] + c <= xv[0]
        y = d["exact"]
        assert y.shape == (n, h, w, ycs) and (nc.bits(y[..., kw * c:]) == 0).all()
        for ox in range(w):
            for dx in range(kw):
                blk = y[:, :, ox, dx * c:(dx + 1) * c]
                if 0 <= ox + dx - pw < w:
                    assert torch.equal(blk, d["x"][:, :, ox + dx - pw])
                else:
                    assert (nc.bits(blk) == 0).all()
        wrong = nc.row_pack_ref(d["x"], kw, pw + 1, ycs)
        assert not torch.equal(wrong, y), name
        print(f"row_pack {name}: pw + 1 moves {int((wrong != y).sum())} of {y.numel()} values")
    assert any(w < kw for _, _, _, w, _, kw, *_ in nc.PACK_CASES)
    assert any(xv[0] > c for _, _, _, _, c, _, _, _, xv in nc.PACK_CASES)
    assert {(c, kw, pw, ycs) for _, _, _, _, c, kw, pw, ycs, _ in nc.PACK_CASES} >= {(3, 7, 3, 32), (6, 7, 3, 64), (5, 3, 0, 16)}
