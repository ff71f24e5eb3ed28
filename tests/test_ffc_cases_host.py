"""CPU checks of what tests/test_ffc_direct_gpu.py feeds the fused FFC kernels (tests/ffc_cases.py): the
(part, channel) references state the model's FourierUnit, the exact sets are exact, the random sets meet the
conditions their tolerances assume, and the case lists reach every argument form.  Run with ``-s`` to see
the transform-rule numbers and the measured conditions per level."""
import pytest
import torch

import ffc_cases as fc

LEVELS = fc.LEVELS


@pytest.mark.parametrize("h", LEVELS)
def test_level_constants(h):
    L = fc.level(h)
    assert (L.h, L.c) in ((12, 1024), (24, 256), (48, 128))
    assert (L.cl, L.cg, L.cc) == (L.c // 4, 3 * L.c // 4, 3 * L.c // 8)
    assert L.f == h * (h // 2 + 1)


@pytest.mark.parametrize("h", LEVELS)
def test_part_channel_references_equal_the_model_layout(h):
    """The FourierUnit of the model, restated in its interleaved channel order (2c + part), against the
    (part, channel) references under the permutation engine/lnet.py applies to the conv's rows, columns and
    BatchNorm vectors: spectrum layout and u within 1e-12."""
    L = fc.level(h)
    n, cc = 2, L.cc
    perm = fc.fu_perm(cc)
    assert sorted(perm.tolist()) == list(range(2 * cc))
    t1 = fc.rand(n, h, h, cc, seed=9000 + h)
    w_model = fc.weight("random", 2 * cc, 2 * cc, 9100 + h)
    sc_model, sh_model = fc.bn_vectors("random", 2 * cc, 9200 + h)
    # what the engine packs: rows, columns and BN vectors taken at perm
    w_pc, sc_pc, sh_pc = w_model[perm][:, perm], sc_model[perm], sh_model[perm]
    st_model, u_model = fc.fourier_unit_model(t1.permute(0, 3, 1, 2), w_model, sc_model, sh_model)
    spec = fc.rfft64(t1)                                                     # [n, F, 2cc]
    spec_model = st_model.permute(0, 2, 3, 1).reshape(n, L.f, 2 * cc)
    d_spec = float((spec - spec_model[..., perm]).abs().max())
    # the inv reference takes float32 operands: feed both the same fp64 spectrum instead
    g = torch.relu(spec @ w_pc.double().t() * sc_pc.double() + sh_pc.double())
    u = fc.irfft64(g, h)
    d_u = float((u - u_model.permute(0, 2, 3, 1)).abs().max())
    print(f"level {h}: max|spec - model| = {d_spec:.2e}, max|u - model| = {d_u:.2e}")
    assert d_spec <= 1e-12 and d_u <= 1e-12
    # and the packaged reference is that same formula
    ref = fc.inv_reference(spec.float(), w_pc, sc_pc, sh_pc, torch.zeros(n, h, h, cc), h)
    g32 = torch.relu(spec.float().double() @ w_pc.double().t() * sc_pc.double() + sh_pc.double())
    assert torch.equal(ref["u"], fc.irfft64(g32, h))
    fwd = fc.fwd_reference(fc.rand(n, h, h, L.cg, seed=1), fc.weight("random", cc, L.cg, 2), None, None)
    assert torch.equal(fwd["spec"], fc.rfft64(fwd["t1"]))


@pytest.mark.parametrize("h", LEVELS)
def test_transform_rule_numbers(h):
    """e_ref, floor and tolerance of the transform rule for every case that uses it, and the separable float32
    form against torch.fft in float64 (it is the same transform: e_ref is rounding, far below a wrong sign or
    table entry, which moves a unit-magnitude spectrum by ~1)."""
    for name, cases, get in (("fwd", fc.FWD_CASES, fc.fwd_case), ("inv", fc.INV_CASES, fc.inv_case)):
        for i, c in enumerate(cases):
            if c.get("only", h) != h:
                continue
            d = get(h, i)
            mag = float((d["spec"] if name == "fwd" else d["u"]).abs().max())
            print(f"level {h} {name} {c['name']}: e_ref={d['e_ref']:.2e} floor={d['floor']:.2e} "
                  f"tol_T={d['tol_t']:.2e} max|ref64|={mag:.2e}")
            assert 0 < d["tol_t"] <= 2e-5 * max(1.0, mag)


def _active(t):
    return float((t > 0).double().mean())


@pytest.mark.parametrize("h", LEVELS)
def test_exact_sets_are_exact(h):
    """The float32 CPU matmul of every exact-set GEMM equals the float64 one bit for bit (every product and
    partial sum is representable), operands are multiples of 1/8 in [-1, 1], and the ReLU behind it is
    active on a fraction in [0.2, 0.8]."""
    def eighth(t):
        return bool(((t.double() * 8) == (t.double() * 8).round()).all() and t.abs().max() <= 1)

    for i, c in enumerate(fc.FWD_CASES):
        if c["kind"] == "exact" and c.get("only", h) == h:
            d = fc.fwd_case(h, i)
            assert eighth(d["x"]) and eighth(d["w"])
            assert torch.equal((d["x"] @ d["w"].t()).double(), d["x"].double() @ d["w"].double().t())
            assert torch.equal(d["t1"].float().double(), d["t1"])
            fr = _active(d["t1"])
            print(f"level {h} fwd {c['name']}: ReLU-active {fr:.3f}")
            assert 0.2 <= fr <= 0.8
    for i, c in enumerate(fc.INV_CASES):
        if c["kind"] == "exact" and c.get("only", h) == h:
            d = fc.inv_case(h, i)
            assert eighth(d["spec"]) and eighth(d["w"])
            assert torch.equal((d["spec"] @ d["w"].t()).double(), d["spec"].double() @ d["w"].double().t())
            assert torch.equal(d["g"].float().double(), d["g"])
            fr = _active(d["g"])
            print(f"level {h} inv {c['name']}: ReLU-active {fr:.3f}")
            assert 0.2 <= fr <= 0.8
    for i, c in enumerate(fc.NORM_CASES):
        if c["kind"] == "exact" and c.get("only", h) == h:
            d = fc.norm_case(h, i)
            cl = d["level"].cl
            assert eighth(d["u"]) and eighth(d["w"]) and eighth(d["yv"])
            v32 = d["yv"].clone()
            v32[..., cl:] += d["u"] @ d["w"].t()
            assert torch.equal(v32.double(), d["v"])
            if c["act"] == "relu":
                fr = _active(d["ref"])
                print(f"level {h} norm {c['name']}: ReLU-active {fr:.3f}")
                assert 0.2 <= fr <= 0.8


@pytest.mark.parametrize("h", LEVELS)
def test_random_sets_meet_their_conditions(h):
    """sigma >= 0.25 for every (image, channel) of every norm case (the condition of the propagated norm
    bound; the exact sets too), ReLU-active fractions of t1 and G in [0.2, 0.8], and inv spectra that are
    not Hermitian-consistent: max|rfftn(irfftn(z)) - z| >= 0.1."""
    for i, c in enumerate(fc.NORM_CASES):
        if c.get("only", h) == h:
            d = fc.norm_case(h, i)
            smin = float(d["std"].min())
            tols = [float(fc.norm_tol(d, p).max()) for p in ("f16x3", "bf16x3")]
            print(f"level {h} norm {c['name']}: min sigma {smin:.3f}, max tol f16x3 {tols[0]:.2e} bf16x3 {tols[1]:.2e}")
            assert smin >= 0.25
    for i, c in enumerate(fc.FWD_CASES):
        if c["kind"] == "random" and c.get("only", h) == h:
            fr = _active(fc.fwd_case(h, i)["t1"])
            print(f"level {h} fwd {c['name']}: ReLU-active {fr:.3f}")
            assert 0.2 <= fr <= 0.8
    for i, c in enumerate(fc.INV_CASES):
        if c["kind"] == "random" and c.get("only", h) == h:
            d = fc.inv_case(h, i)
            fr = _active(d["g"])
            back = fc.rfft64(fc.irfft64(d["g"], h))
            herm = float((back - d["g"]).abs().max())
            print(f"level {h} inv {c['name']}: ReLU-active {fr:.3f}, max|rfftn(irfftn(z)) - z| = {herm:.3f}, "
                  f"max tol_u f16x3 {float(fc.inv_tol(d, 'f16x3').max()):.2e} "
                  f"bf16x3 {float(fc.inv_tol(d, 'bf16x3').max()):.2e}")
            assert 0.2 <= fr <= 0.8
            assert herm >= 0.1
            assert float(d["t1"].abs().max()) > 0.5                     # the + t1 residual is visible


@pytest.mark.parametrize("h", LEVELS)
def test_case_lists_cover_every_argument_form(h):
    """Per level: an image count that is no multiple of 8, n = 16 (and n = 8 at one level: the XCD-grouped
    block order), both presence states of every optional argument, a wide and a dense pitch of every strided
    one."""
    for cases in (fc.FWD_CASES, fc.INV_CASES, fc.NORM_CASES):
        ns = {c["n"] for c in fc.cases_of(cases, h)}
        assert 16 in ns and any(n % 8 for n in ns)
        assert any(c["n"] == 8 for lv in LEVELS for c in fc.cases_of(cases, lv))
        assert all(c["n"] <= 16 for c in cases)
        if cases is not fc.NORM_CASES:                                      # scale / shift present and absent
            for kind in ("random", "exact"):
                assert {c["bn"] for c in fc.cases_of(cases, h) if c["kind"] == kind} == {True, False}
    fwd = fc.cases_of(fc.FWD_CASES, h)
    assert {c["xf"] for c in fwd} == {"wide", "dense"}
    norm = fc.cases_of(fc.NORM_CASES, h)
    assert {c["gb"] for c in norm} == {None, "halves", "dense"}             # absent, gb_ns = 2C, gb_ns = C
    assert {c["act"] for c in norm} == {"none", "relu", "lrelu"}
    assert {c["eps"] for c in norm} == {1e-5, 1e-3}
    assert {c["y"] for c in norm} >= {"out", 0, 4}                           # in place, dense, wide
    assert {c["out"] for c in norm} == {0, 4}
    assert {c["res"] for c in norm} >= {None, "out", 0, 4}
    assert {c["pad"] for c in norm} == {None, 0, 4}
    assert all(p % 4 == 0 for c in norm for p in (c["y"], c["out"], c["res"], c["pad"]) if isinstance(p, int))
    assert {c["kind"] for c in norm} == {"random", "exact"}
    assert len(fc.X_SCALES) == 2 and min(fc.X_SCALES) < 1 < max(fc.X_SCALES)
