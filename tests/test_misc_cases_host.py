"""CPU checks of the inputs that tests/test_misc_ops_gpu.py feeds the small non-conv kernels: the
cases must reach the paths and edges they are listed for, whatever the kernels then do with them."""
import torch

import misc_cases as mc


def test_warp_cases_cover_taps_and_block_counts():
    """Over the case list: >= 50 % of the output pixels have all four bilinear taps inside the image,
    >= 5 % one to three taps outside, >= 2 % all four outside (from the fp64 sample coordinates); the
    block counts cover nb < 8, nb % 8 == 0, nb > 8 with nb % 8 != 0, and a ragged last block."""
    counts = torch.zeros(5, dtype=torch.int64)
    for i, case in enumerate(mc.WARP_CASES):
        h, w = case[3], case[4]
        counts += torch.bincount(mc.warp_taps_outside(mc.warp_case(i)["flow"], h, w).flatten(), minlength=5)
    frac = counts.double() / counts.sum()
    print("taps outside 0..4:", [f"{f:.3f}" for f in frac.tolist()])
    assert frac[0] >= 0.50
    assert frac[1:4].sum() >= 0.05
    assert frac[4] >= 0.02
    nbs = [mc.warp_blocks(c) for c in mc.WARP_CASES]
    assert any(nb < 8 for nb in nbs)
    assert any(nb % 8 == 0 for nb in nbs)
    assert any(nb > 8 and nb % 8 for nb in nbs)
    assert any((c[1] * c[3] * c[4]) % 256 for c in mc.WARP_CASES)
    # flow at image size and resized flow, per-axis ratios that differ, the smallest legal flow
    assert any((c[5], c[6]) == (c[3], c[4]) for c in mc.WARP_CASES)
    assert any(c[5] * c[4] != c[6] * c[3] and (c[5], c[6]) != (c[3], c[4]) for c in mc.WARP_CASES)
    assert any((c[5], c[6]) == (2, 2) for c in mc.WARP_CASES)
    for form in range(8, 11):
        assert len({c[form] for c in mc.WARP_CASES}) >= 2


def test_warp_patch_is_exactly_zero_in_the_reference():
    i = [c[0] for c in mc.WARP_CASES].index("patch")
    d = mc.warp_case(i)
    n, c = d["src"].shape[:2]
    patch = d["patch"].expand(n, c, -1, -1)
    assert patch.any() and not patch.all()
    assert d["flow"].abs().max() < 1e6 and torch.isfinite(d["flow"]).all()
    assert (d["ref64"][patch] == 0).all() and (d["ref32"][patch] == 0).all()
    assert (d["ref64"][~patch] != 0).float().mean() > 0.5


def test_warp_references_are_fp32_close():
    """The fp32 reference error stays far below the ~0.1 of a wrong tap: e_ref <= 1e-4 per case."""
    for i in range(len(mc.WARP_CASES)):
        d = mc.warp_case(i)
        print(f"warp {d['name']}: e_ref={d['e_ref']:.2e} zero fraction={(d['ref64'] == 0).float().mean():.3f}")
        assert 0 < d["tol"] <= 4e-4


def test_attention_cases_reach_overflowing_logits():
    """exp() of an fp32 logit above 88.7 is inf: the magnitude-12 case has logits far beyond it (an
    evaluation without the row-max subtraction cannot pass), the magnitude-6 case about +-50."""
    by_mag = {c[3]: mc.attn_case(i) for i, c in enumerate(mc.ATTN_CASES) if c[3] > 1}
    assert by_mag[12.0]["max_logit"] > 150
    assert 30 < by_mag[6.0]["max_logit"] < 88
    for i, (b, T, heads, _) in enumerate(mc.ATTN_CASES):
        d = mc.attn_case(i)
        print(f"attention {mc.ATTN_CASES[i]}: e_ref={d['e_ref']:.2e} floor={d['floor']:.2e} "
              f"max|logit|={d['max_logit']:.1f}")
        assert T <= 256 and d["tol"] <= 1e-4
        if T == 1:
            assert torch.equal(d["ref64"], d["v"].double())
    assert any(T == 256 for _, T, _, _ in mc.ATTN_CASES) and any(T < 4 for _, T, _, _ in mc.ATTN_CASES)
    assert any(T % 64 == 1 and T > 64 for _, T, _, _ in mc.ATTN_CASES)


def test_layernorm_cases():
    for i, (rows, dim, off, spread) in enumerate(mc.LN_CASES):
        d = mc.ln_case(i)
        print(f"row_layernorm {mc.LN_CASES[i]}: e_ref={d['e_ref']:.2e} floor={d['floor']:.2e}")
        if dim == 1:
            assert torch.equal(d["ref64"], d["b"].double().expand(rows, 1))
        assert d["tol"] < 2e-2
    assert any(r % 4 for r, *_ in mc.LN_CASES)
    assert any(d < 64 for _, d, *_ in mc.LN_CASES) and any(d > 64 and d % 64 for _, d, *_ in mc.LN_CASES)


def test_eltwise_fp32_evaluation_is_within_half_the_bound():
    """The plain CPU fp32 evaluation of every eltwise case stays within half of the per-element bound
    the GPU test asserts, and the pre-activation values sample about [-6, 6]."""
    lo, hi = 0.0, 0.0
    for i, spec in enumerate(mc.ELT_CASES):
        d = mc.elt_case(i)
        err = (d["ref32"].double() - d["ref64"]).abs()
        ratio = float((err / d["bound"]).max())
        assert ratio <= 0.5, (spec["name"], ratio)
        if spec["mul"] is not None and spec["add"] is not None and spec["bias"] is not None and d["a"] == 1.0:
            v = d["x"].double() * d["mul"].double() + d["add"].double() + d["bias"].double()
            lo, hi = min(lo, float(v.min())), max(hi, float(v.max()))
    assert lo < -5.0 and hi > 5.0, (lo, hi)


def test_eltwise_case_list_covers_the_issue():
    names = [c["name"] for c in mc.ELT_CASES]
    assert len(set(names)) == len(names)
    for lay in "ab":
        for act in mc.ACTS:
            assert f"{lay}-{act}" in names
        assert sum(n.startswith(f"{lay}-mul") for n in names) == 8
    c8 = mc._LAYOUT["a"]
    assert c8["c"] % 4 == 0 and all(p % 4 == 0 and o % 4 == 0 for p, o in (c8["x"], c8["y"], c8["mul"], c8["add"]))
    assert mc._LAYOUT["b"]["c"] % 4
    n, h, w = mc.ELT_NHW
    assert (n * h * w) % 64


def test_amax_case_list():
    for i, (name, nhw, c, pitch, off) in enumerate(mc.AMAX_CASES):
        t = mc.amax_base(i)
        assert t.shape == nhw + (pitch,) and off + c <= pitch
        view = t[..., off:off + c]
        assert view.abs().max() <= 1.0 < mc.AMAX_PEAK < mc.AMAX_NEIGHBOUR
        if pitch > c:
            assert t.abs().max() == mc.AMAX_NEIGHBOUR
    px = {name: nhw[0] * nhw[1] * nhw[2] for name, nhw, *_ in mc.AMAX_CASES}
    assert px["c256-8197px"] > 2048 * 4 and px["c1-524289px"] > 2048 * 256
