"""The opt-in single-pass f16 conv arithmetic ("f16", S2V_PREC_F16) on the device.

Each product is f16(a) * f16(b), both rounded to nearest even, accumulated in fp32 by one
v_mfma_f32_16x16x32_f16 per fragment pair (conv_igemm_x3 / conv_x3_halo ELT 2).  The mode is OUTSIDE the fp32
parity bar by design; these tests pin what it is instead:
  1. exact on operands that f16 represents (no lo slot read, no fragment from the wrong half, no K-slice missed);
  2. equal to the fp64 conv of the f16-rounded operands up to the fp32 sums (one pass, nearest even), on a
     fixture that the three-pass f16x3 result provably fails;
  3. within 1e-3 sum|a b| of the unrounded conv ((1 + 2^-11)^2 - 1 = 9.77e-4 per product);
  4. covered by the f16 range guard as f16x3 is;
  5. the models against the reference goldens at twice the error measured on MI355X
     (profiles/f16_precision.json), which must stay below 3x the CPU emulation of the mode;
  6. selectable per clip (inference.run(precision=), captured graphs keep it).
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import s2v_import  # noqa: F401
import f16_cases as C
from f16_cases import CASES, DEV, REL_F16, REL_F32

pytestmark = pytest.mark.gpu

from s2v_amd import _lib, ops  # noqa: E402
from s2v_amd.ops import NHWC, ConvW  # noqa: E402


@pytest.fixture(scope="module")
def ctx():
    return ops.Ctx(DEV)


@pytest.fixture(scope="module")
def rnd_refs():
    """Per case, computed once: the rnd inputs of test_conv2d, their weights and the fp64 references."""
    out = {}
    for case in CASES:
        x, ws = C.inputs(case, False), C.weights(case, False)
        out[case.name] = (x, ws, C.reference(case, x, ws))
    return out


def _plans(ctx, case, x, cws):
    """The plans of the case's launches (ops.CONV_HOOK; a hook makes a conv group launch member by member)."""
    plans = []

    def hook(c, p, flops, go):
        plans.append(p.plan)
        go()
    ops.CONV_HOOK = hook
    try:
        C.launch(ctx, case, x, cws)
    finally:
        ops.CONV_HOOK = None
    return plans


@pytest.mark.parametrize("case", CASES, ids=repr)
@pytest.mark.parametrize("relu", [False, True], ids=["none", "relu"])
def test_exact_on_representable_operands(ctx, case, relu):
    """x = k / 8, w = m / 16, bias = j / 128: every product and partial sum is exact in fp32 (sum|ab| <= 9216 at the
    largest K here, in steps of 2^-7: < 2^24 steps), so the output EQUALS the fp64 conv in any summation order."""
    x, ws = C.inputs(case, True), C.weights(case, True)
    refs = C.reference(case, x, ws)
    cws = C.conv_weights(case, ws)
    with ops.precision("f16"):
        ops.LAST_GROUP = None
        got = C.launch(ctx, case, x, cws, epi=lambda i, s: dict(act=ops.ACT_RELU) if relu else {})
        if case.group:
            assert ops.LAST_GROUP == 1                       # one grouped kernel (conv_igemm_x3_group ELT 2)
        elif not relu:
            plans = _plans(ctx, case, x, cws)
            assert len(plans) == 1 and plans[0][6] == 3, plans   # the launch really ran single-pass
            assert plans[0][10] == case.cap, plans
            sym = ops.plan_symbol(plans[0])
            assert sym.startswith("void s2v::conv_x3_halo<2, ") or sym.endswith(", 2>(s2v::ConvArgs)"), sym
            assert ("persist" in sym) == bool(case.cap), sym
    for g, (ref, bound) in zip(got, refs):
        assert float(bound.max()) * 128 < 2 ** 24
        exp = F.relu(ref) if relu else ref
        assert torch.equal(g, exp), f"max diff {(g - exp).abs().max():.3e} at {int((g != exp).sum())} outputs"


@pytest.mark.parametrize("case", CASES, ids=repr)
def test_one_pass_rounded_to_nearest_even(ctx, case, rnd_refs):
    """got == conv64(f16(x), f16(w 2^s) / 2^s) + bias up to the fp32 sums (REL f32 of tests/test_ops_gpu.py), with s
    the packer's weight pre-scale exponent; the f16x3 output of the same launch violates that bound by > 4x, so a
    mode that silently ran three passes fails here."""
    x, ws, _ = rnd_refs[case.name]
    cws = C.conv_weights(case, ws)
    scales = [cw.split_scale(ops.PREC_F16) for cw in cws]
    assert all(s == cw.split_scale(ops.PREC_F16X3) and s > 1.0 for s, cw in zip(scales, cws))
    ref16 = C.reference(case, x, ws, xmap=lambda t: t.float().half().double(),
                        wmap=lambda w, i: (w.float() * scales[i]).half().double() / scales[i])
    with ops.precision("f16"):
        got = C.launch(ctx, case, x, cws)
    with ops.precision("f16x3"):
        got3 = C.launch(ctx, case, x, cws)
    for g, g3, (ref, bound) in zip(got, got3, ref16):
        lim = REL_F32 * (bound + 1) + 1e-6
        err, err3 = (g - ref).abs(), (g3 - ref).abs()
        print(f"{case.name}: f16 max err/lim {float((err / lim).max()):.3f}, f16x3 max err/lim "
              f"{float((err3 / lim).max()):.1f}, share > 4 lim {float((err3 > 4 * lim).double().mean()):.2f}")
        assert (err <= lim).all(), f"max err {err.max():.3e}, err/lim {(err / lim).max():.2f}"
        assert float((err3 / lim).max()) > 4, "the fixture does not tell one pass from three"


@pytest.mark.parametrize("case", CASES, ids=repr)
def test_bound_against_the_unrounded_conv(ctx, case, rnd_refs):
    """|got - conv64(x, w)| <= 1e-3 (sum|x||w| + 1) + 1e-6 through the three epilogues of test_conv2d: bias + lrelu;
    nc_scale + residual-before + sigmoid; residual-after + tanh into a slice of a wider tensor."""
    x, ws, refs = rnd_refs[case.name]
    cws = C.conv_weights(case, ws)
    shapes = [r.shape for r, _ in refs]
    res = [C.rnd(*s, seed=4 + i) for i, s in enumerate(shapes)]
    ncs = [C.rnd(s[0], s[1], seed=5 + i, lo=0.5, hi=1.5) for i, s in enumerate(shapes)]

    def nhwc(t):
        return NHWC(t.float().permute(0, 2, 3, 1).contiguous().to(DEV))
    # on the device before the launches, alive until they ran (a conv group launches at the end of its block)
    res_d, ncs_d = [nhwc(r) for r in res], [s.float().to(DEV) for s in ncs]
    for variant in range(3):
        def epi(i, shape):
            if variant == 0:
                return dict(act=ops.ACT_LRELU, alpha=0.2)
            if variant == 1:
                return dict(act=ops.ACT_SIGMOID, res=res_d[i], nc_scale=ncs_d[i])
            return dict(act=ops.ACT_TANH, res=res_d[i], res_after=True)
        with ops.precision("f16"):
            got = C.launch(ctx, case, x, cws, epi=epi, wide=variant == 2)
        for i, (g, (ref, bound)) in enumerate(zip(got, refs)):
            b = ws[i][1][None, :, None, None]
            if variant == 0:
                exp = F.leaky_relu(ref, 0.2)
            elif variant == 1:
                exp = torch.sigmoid((ref - b) * ncs[i][:, :, None, None] + b + res[i])
            else:
                exp = torch.tanh(ref) + res[i]
            err = (g - exp).abs()
            lim = REL_F16 * (bound + 1) + 1e-6
            print(f"{case.name} variant {variant}: max err/lim {float((err / lim).max()):.3f}")
            assert (err <= lim).all(), f"variant {variant}: max err {err.max():.3e}, err/lim {(err / lim).max():.2f}"


# ----------------------------------------------------------------------------- range guard (as tests/test_range_gpu.py)
@pytest.mark.parametrize("mag", [6e4, 1e-6])
def test_conv_inputs_outside_the_f16_range(mag):
    """A layer whose input lies at the f16 ceiling / far below the normal range gets the calibrated power-of-two
    pre-scale in "f16" mode too and stays within the per-product bound, relative to sum|x||w| alone."""
    g = torch.Generator().manual_seed(1)
    x = (torch.rand(2, 64, 13, 11, generator=g, dtype=torch.float64) * 2 - 1) * mag
    wt = torch.randn(96, 64, 3, 3, generator=g, dtype=torch.float64) / 24
    c = ops.Ctx(DEV)
    cw = ConvW(wt.float(), None, DEV, padding=1)
    y = NHWC.empty(2, 13, 11, 96, DEV)
    with ops.precision("f16"):
        assert ops.guard_active()
        ops.conv2d(c, NHWC(x.permute(0, 2, 3, 1).float().contiguous().to(DEV)), cw, y)
        c.check_range()
    got = y.t.permute(0, 3, 1, 2).double().cpu()
    ref = F.conv2d(x.float().double(), wt.float().double(), None, 1, 1)
    bound = F.conv2d(x.float().double().abs(), wt.float().double().abs(), None, 1, 1)
    assert torch.isfinite(got).all()
    assert ((got - ref).abs() <= REL_F16 * bound + 1e-30).all(), float(((got - ref).abs() / (bound + 1e-30)).max())
    expect = ops.x_scale_for(float(x.float().abs().max()))
    assert cw._xscale[ops.PREC_F16] == expect and expect != 1.0


def test_overflow_after_calibration_is_flagged():
    g = torch.Generator().manual_seed(2)
    x = torch.rand(2, 64, 13, 11, generator=g) * 2 - 1
    cw = ConvW(torch.randn(96, 64, 3, 3, generator=g) / 24, None, DEV, padding=1)
    c = ops.Ctx(DEV)
    y = NHWC.empty(2, 13, 11, 96, DEV)
    with ops.precision("f16"):
        ops.conv2d(c, NHWC((x * 10).permute(0, 2, 3, 1).contiguous().to(DEV)), cw, y)     # calibrates: no pre-scale
        c.check_range()
        ops.conv2d(c, NHWC((x * 1e6).permute(0, 2, 3, 1).contiguous().to(DEV)), cw, y)
        with pytest.raises(_lib.S2VError, match="non-finite"):
            c.check_range()
        c.check_range()


def test_model_forward_out_of_range_batch_reruns_in_bf16x3():
    """An LNet batch that leaves the range its "f16" calibration measured sets the lane's non-finite flag and runs
    again in bf16x3: the output equals a bf16x3 forward bit for bit; forwards that stay in range do not re-run.

    The issue asked for a batch 1e3 x outside the calibrated range.  Measured on MI355X, a face input 1e3 x larger
    stays inside the f16 range everywhere in LNet (largest operand 1e3 at the first conv, the norms behind it undo the
    factor): no accumulator is non-finite, so nothing is flagged and re-running would be wrong; the same holds in
    f16x3.  That case is kept as an in-range case (no re-run, finite output), and the re-run is checked at 1e5 x, the
    factor tests/test_range_gpu.py uses for the same property."""
    net = C.build_model("lnet")
    g = torch.Generator(device=DEV).manual_seed(7)
    mel = torch.rand((2, 1, 80, 16), generator=g, device=DEV) * 8 - 4
    face = torch.rand((2, 6, 96, 96), generator=g, device=DEV)
    with ops.precision("f16"):
        net(mel, face)                                       # first forward: calibration
        eng, lanes = net._s2v_engines[str(face.device)]
        assert "f16" in eng.__dict__["_calibrated"]          # its own calibration entry
        c = lanes[0]
        assert c.reruns == 0
        ok = net(mel, face)
        assert c.reruns == 0 and torch.isfinite(ok).all()
        mid = net(mel, face * 1.0e3)                         # inside the f16 range: stays "f16"
        assert c.reruns == 0 and torch.isfinite(mid).all()
        big = face * 1.0e5
        out = net(mel, big)
        assert c.reruns == 1 and torch.isfinite(out).all()
    with ops.precision("bf16x3"):
        ref = net(mel, big)
    assert torch.equal(out, ref)


# ----------------------------------------------------------------------------- models against the reference goldens
# CPU emulation of the mode on the reference math (f16_cases.emulation_figures: every conv operand of the oracle
# rounded to 11 bits), (max, mean) |emulated - plain| per output; recorded in profiles/f16_precision.json
EMULATED = {
    "lnet_out": (1.08e-2, 1.8e-3), "enet_out_clamped": (1.9e-2, 6.9e-6), "enet_out": (1.07e-1, 1.07e-2),
    "enet_low": (1.0e-2, 1.4e-3), "dnet_flow": (4.4e-3, 6.6e-4), "dnet_warp_image": (1.87e-2, 1.5e-3),
    "dnet_fake_image": (2.2e-2, 1.6e-3), "gfpgan_out": (7.4e-2, 1.04e-2), "gfpgan_rgb0": (1.36e-3, 3.5e-4),
    "gfpgan_rgb3": (5.3e-3, 1.4e-3),
}
# measured on MI355X against the goldens (profiles/f16_precision.json "device"): (max, mean)
MEASURED = {
    "lnet_out": (1.499e-2, 2.380e-3), "enet_out": (1.292e-1, 1.122e-2), "enet_out_clamped": (1.783e-2, 5.425e-6),
    "enet_low": (1.212e-2, 1.838e-3), "dnet_flow": (6.886e-3, 1.111e-3), "dnet_warp_image": (3.276e-2, 2.475e-3),
    "dnet_fake_image": (3.305e-2, 2.711e-3), "gfpgan_out": (5.314e-2, 9.641e-3), "gfpgan_rgb0": (9.831e-4, 3.335e-4),
    "gfpgan_rgb3": (3.840e-3, 1.228e-3),
}
FALLBACK = ("conv_x3_nar<1,", "conv_head_x3<1,", "conv_glds_x3<")            # families that run "f16" as f16x3
EXACT = ("conv_k4_mfma<", "conv_smallk<", "conv_smallk4<", "conv_halo_small<", "conv_small_cpar<",
         "conv_direct_small<")                                                # exact fp32 in every mode


def _round_up(v):
    """v rounded up to one significant digit."""
    e = 10.0 ** np.floor(np.log10(v))
    return float(np.ceil(v / e - 1e-9) * e)


TOL = {"f16": {k: (_round_up(2 * m), _round_up(2 * mean)) for k, (m, mean) in MEASURED.items()}}


@pytest.mark.parametrize("model", ["lnet", "enet", "dnet", "gfpgan"])
def test_models_against_the_reference_goldens(model, golden):
    g = golden(C.GOLDEN_OF[model])
    net = C.build_model(model)
    with ops.precision("f16"):
        outs = C.device_outputs(model, net)
        launches = []

        def hook(c, p, flops, go):
            launches.append((p.plan[6], ops.plan_symbol(p.plan), flops))
            go()
        ops.CONV_HOOK = hook
        try:
            C.device_outputs(model, net)
        finally:
            ops.CONV_HOOK = None
    for key, t in outs.items():
        m, mean = C.golden_error(key, t, g)
        print(f"{key}: max {m:.3e} mean {mean:.3e}")
        assert key in MEASURED, f"{key}: no measured figure recorded"
        # plausibility: nothing but operand rounding contributes (below 3x the CPU emulation of the mode)
        if key in EMULATED:
            assert MEASURED[key][0] < 3 * EMULATED[key][0], (key, MEASURED[key], EMULATED[key])
        assert m <= TOL["f16"][key][0] and mean <= TOL["f16"][key][1], (key, m, mean, TOL["f16"][key])
    # the forward really ran single-pass plans; everything else is a fallback family (as f16x3) or exact fp32
    assert any(p == 3 for p, _, _ in launches)
    for p, sym, _ in launches:
        name = sym[len("void s2v::"):]
        if p == 3:
            assert name.startswith(("conv_igemm_x3<", "conv_igemm_x3_persist<", "conv_x3_halo<2, ")), sym
        elif p == 2:
            assert name.startswith(FALLBACK), sym
        else:
            assert p == 0 and name.startswith(EXACT), sym
    f3 = sum(f for p, _, f in launches if p == 3)
    print(f"{model}: {100 * f3 / sum(f for _, _, f in launches):.1f} % of the conv FLOPs ran single-pass")


# ----------------------------------------------------------------------------- pipeline and CLI
@pytest.fixture(scope="module")
def clip():
    """The 8-frame examples fixture and its run in the process default arithmetic (shared by the two tests below)."""
    import os
    from conftest import GOLDEN
    from s2v_amd import inference
    face, wav = os.path.join(GOLDEN, "examples", "face_1.mp4"), os.path.join(GOLDEN, "examples", "audio_1.wav")
    return face, wav, ops.PRECISION, inference.run(face, wav, max_frames=8)


def test_inference_run_under_the_mode(clip):
    """inference.run(precision="f16") on the 8-frame examples fixture: uint8 frames that differ from the f16x3 run's, by
    no more than the model bound x 255 + 1 levels; meta names the arithmetic; ops.PRECISION is restored.

    The model bound is ENet's raw output bound TOL["f16"]["enet_out"]: a frame is clamp(out, 0, 1) * 255 and
    |clamp(a) - clamp(b)| <= |a - b|, so the unclamped bound holds for any clip, whereas the clamped figure of the golden
    input (1.8e-2) is that small only because the golden output saturates outside [0, 1] almost everywhere.  Measured on
    MI355X: 38 levels at the worst pixel of this clip (0.8 on average, 2 % of the pixels above 8), whose predictions lie
    inside [0, 1]; on a saturating clip the same chain differs by 5 levels (DNet's reference frame by 6, ENet on equal
    inputs by 3.7)."""
    from s2v_amd import inference
    face, wav, prev, base = clip
    fast = inference.run(face, wav, max_frames=8, precision="f16")
    assert ops.PRECISION == prev                             # restored
    assert fast["meta"]["conv_arith"] == "f16" and base["meta"]["conv_arith"] == prev
    assert fast["frames"].dtype == torch.uint8 and fast["frames"].shape == base["frames"].shape
    assert fast["meta"]["frames"] == 8
    d = (fast["frames"].int() - base["frames"].int()).abs()
    bound = TOL["f16"]["enet_out"][0] * 255 + 1
    print(f"frames: {int((d > 0).sum())} pixels differ, max {int(d.max())} levels (bound {bound:.1f})")
    assert int(d.max()) >= 1 and int(d.max()) <= bound


def test_inference_run_without_precision_is_unchanged(clip):
    """Naming the process default explicitly gives the bytes of the call without ``precision``."""
    from s2v_amd import inference
    face, wav, prev, base = clip
    same = inference.run(face, wav, max_frames=8, precision=prev)
    assert ops.PRECISION == prev
    assert torch.equal(same["frames"], base["frames"]) and torch.equal(same["preds"], base["preds"])


def test_replayed_batch_keeps_the_precision_it_was_captured_with():
    from test_pipeline_gpu import _clip
    from s2v_amd import audio, pipeline as P
    dnet, enet = C.build_model("dnet"), C.build_model("enet")
    wav, semantic, expression, src = _clip(4, 4)
    chunks = audio.mel_chunks(audio.melspectrogram(torch.from_numpy(wav).to(DEV)))
    coeffs = torch.from_numpy(P.dnet_coefficients(semantic[:4], expression)).to(DEV)
    pipe = P.LipSyncPipeline(dnet, enet, DEV, batch=2)                    # two replayed batches
    with ops.precision("f16"):
        first = pipe.run(chunks, src[:4].to(DEV), coeffs, 0, 4)
    assert ops.PRECISION != "f16"
    again = pipe.run(chunks, src[:4].to(DEV), coeffs, 0, 4)               # replays the graphs captured under "f16"
    assert pipe.reruns == 0 and torch.equal(first, again)
    other = P.LipSyncPipeline(dnet, enet, DEV, batch=2).run(chunks, src[:4].to(DEV), coeffs, 0, 4)
    assert not torch.equal(other, first)                                  # the process default computes other frames
