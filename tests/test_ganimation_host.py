"""GANimation upper-face editing, host side: the parameter mirror and loader, the weight transformations of
engine/ganimation.py against torch's own convolutions on the CPU, the engine's host plan, the argument checks of
the pipeline, the CLI and the C ABI, and the restatement of inference.py:277-288 (tests/ganimation_cases.py)
against the probes tests/golden/make_ganimation_golden.py recorded from the reference's SplitGenerator."""
import ctypes
import inspect
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import s2v_import  # noqa: F401
import ganimation_cases as GC

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def sd():
    return GC.state_dict()


def test_state_dict_manifest_is_the_references(sd):
    from s2v_amd.models.ganimation_arch import SplitGeneratorParams
    with open(os.path.join(GOLDEN, "ganimation_keys.json")) as f:
        want = json.load(f)
    assert len(want) == 36
    mine = {k: list(v.shape) for k, v in SplitGeneratorParams().state_dict().items()}
    assert mine == want
    assert list(mine)[:2] == ["model.0.weight", "model.0.bias"] and "model.18.bias" in mine
    assert mine["color_top.0.weight"] == [3, 64, 7, 7] and mine["au_top.0.weight"] == [1, 64, 7, 7]
    assert mine["model.15.weight"] == [256, 128, 4, 4]                    # ConvTranspose2d: [in, out, k, k]
    with pytest.raises(NotImplementedError):
        SplitGeneratorParams(n_blocks=9)


def test_load_ganimation_strips_filters_and_raises(tmp_path, sd):
    from s2v_amd import ganimation, models
    wrapped = {"module." + k: v for k, v in sd.items()}
    wrapped["module.extra.weight"] = torch.zeros(3)                       # unknown keys are dropped (base_model.py:133)
    torch.save(wrapped, tmp_path / "30_net_gen.pth")
    net = models.load_ganimation(str(tmp_path / "30_net_gen.pth"))
    assert not net.training
    assert all(torch.equal(v, sd[k]) for k, v in net.state_dict().items()) and len(net.state_dict()) == 36
    torch.save({k: v for k, v in sd.items() if k != "model.12.conv_block.3.bias"}, tmp_path / "bad.pth")
    with pytest.raises(RuntimeError, match="model.12.conv_block.3.bias"):
        models.load_ganimation(str(tmp_path / "bad.pth"))
    with pytest.raises(FileNotFoundError):
        models.load_ganimation(str(tmp_path / "absent.pth"))
    with pytest.raises(FileNotFoundError, match="absent"):                # never downloads
        ganimation.GANimationModel().initialize(str(tmp_path / "absent.pth"))
    m = ganimation.GANimationModel().initialize(str(tmp_path / "30_net_gen.pth")).setup()
    assert m.models_name == ["gen"] and m.is_train is False and m.name == "GANimation"


def test_exp_aus_dict_is_the_references():
    from s2v_amd import ganimation
    d = ganimation.exp_aus_dict
    assert sorted(d) == ["angry", "sad", "surprise"] and ganimation.GANimationModel.exp_aus_dict is d
    want = {"sad": {}, "angry": {2: 0.3}, "surprise": {3: 0.2}}           # AU04 = 0.3; AU05 = 0.2
    for name, t in d.items():
        ref = torch.zeros(1, 17)
        for i, v in want[name].items():
            ref[0, i] = v
        assert t.dtype == torch.float32 and torch.equal(t, ref), name
    assert ganimation.check_up_face("angry") == "angry"
    for bad in ("original", "happy", None):
        with pytest.raises(ValueError, match="up_face"):
            ganimation.check_up_face(bad)


def _unpack(cw):
    """ConvW's packed [npad][kpad] weights back to [O, I, kh, kw]."""
    return cw.wt[: cw.cout, : cw.K].reshape(cw.cout, cw.kh, cw.kw, cw.cin).permute(0, 3, 1, 2)


def test_stacked_head_and_polyphase_classes_equal_torch(sd):
    """The engine's two weight transformations as plain torch convolutions on the CPU: the stacked head is
    cat(color_top, au_top), and the four parity classes of each transposed stage, written with step 2,
    are conv_transpose2d."""
    from s2v_amd.engine.ganimation import GANimationEngine
    eng = GANimationEngine(sd, "cpu")
    g = torch.Generator().manual_seed(11)
    x = torch.randn((2, 64, 9, 7), generator=g).double()
    head = F.conv2d(x, _unpack(eng.head).double(), padding=3)
    assert head.shape == (2, 4, 9, 7) and (eng.head.scale, eng.head.shift) == (None, None)
    assert (eng.head.ph, eng.head.pw, eng.head.sh, eng.head.sw) == (3, 3, 1, 1)
    assert torch.equal(_unpack(eng.head), torch.cat([sd["color_top.0.weight"], sd["au_top.0.weight"]]))
    assert (head[:, :3] - F.conv2d(x, sd["color_top.0.weight"].double(), padding=3)).abs().max() < 1e-12
    assert (head[:, 3:] - F.conv2d(x, sd["au_top.0.weight"].double(), padding=3)).abs().max() < 1e-12
    for cw, idx in zip(eng.up, (15, 18)):
        w = sd[f"model.{idx}.weight"]
        x = torch.randn((2, w.shape[0], 5, 6), generator=g)
        ref = F.conv_transpose2d(x.double(), w.double(), stride=2, padding=1)
        out = torch.zeros_like(ref)
        assert len(cw.poly) == 4 and cw.out_hw(5, 6) == (10, 12)
        for (ry, rx), sub, _ in cw.poly:
            assert (sub.kh, sub.kw) == (2, 2)                              # each parity class has 2x2 taps
            # the class's padding is its top / left reach; rows and columns past the input read zero
            xp = F.pad(x.double(), (sub.pw, 2, sub.ph, 2))
            out[:, :, ry::2, rx::2] = F.conv2d(xp, _unpack(sub).double())[:, :, : (10 - ry + 1) // 2,
                                                                         : (12 - rx + 1) // 2]
        assert (out - ref).abs().max() < 1e-12


def test_engine_plan_runs_dry(monkeypatch, sd):
    """Shapes, views and launch counts on the CPU with no-op launches; sizes off the multiple of 4 raise before
    any launch."""
    from test_engine_dryrun import _NoLib, _NoOps
    from s2v_amd import ops
    from s2v_amd.engine import ganimation as EG
    lib = _NoLib()
    monkeypatch.setattr(ops, "S2V", _NoOps(lib.calls))
    monkeypatch.setattr(ops, "_require_cuda", lambda t, what: None)
    monkeypatch.setattr(ops._lib, "load", lambda: lib)
    monkeypatch.setattr(ops.Ctx, "stream", property(lambda self: ctypes.c_void_p(0)))
    eng = EG.GANimationEngine(sd, "cpu")
    ctx = ops.Ctx("cpu")
    with ops.precision("f32"):
        head, embed = eng.forward(ctx, ops.NHWC(torch.zeros(2, 44, 36, 20)))
    assert (head.n, head.h, head.w, head.cs) == (2, 44, 36, 4) and (embed.h, embed.w, embed.c) == (44, 36, 64)
    assert (EG.CONVS, EG.NORMS, EG.LAUNCHES) == (24, 17, 41)
    assert lib.calls["conv2d_"] == EG.CONVS and lib.calls["instnorm_"] == EG.NORMS
    before = dict(lib.calls)
    for hw in ((42, 36), (44, 38), (0, 4)):
        with pytest.raises(ValueError, match="multiples of 4"):
            eng.forward(ctx, ops.NHWC(torch.zeros(1, *hw, 20)))
    with pytest.raises(ValueError, match="channels"):
        eng.forward(ctx, ops.NHWC(torch.zeros(1, 8, 8, 4)))
    assert lib.calls == before


def test_pipeline_and_cli_arguments():
    from s2v_amd import inference, pipeline as P
    ap = inference.build_parser()
    a = ap.parse_args(["--face", "v.mp4", "--audio", "a.wav"])
    assert (a.up_face, a.without_rl1) == ("original", False)              # the reference's names and defaults
    a = ap.parse_args(["--face", "v.mp4", "--audio", "a.wav", "--up_face", "surprise", "--without_rl1"])
    assert (a.up_face, a.without_rl1) == ("surprise", True)
    sig = inspect.signature(inference.run).parameters
    assert sig["up_face"].default == "original" and sig["without_rl1"].default is False
    with pytest.raises(ValueError, match="up_face"):                      # before any file is read or launch made
        inference.run("absent.mp4", "absent.wav", up_face="happy", device="cpu")
    sig = inspect.signature(P.LipSyncPipeline.__init__).parameters
    assert sig["up_face"].default is None and sig["without_rl1"].default is False
    assert "orig_u8" in inspect.signature(P.LipSyncPipeline.run).parameters
    assert "orig_u8" in inspect.signature(P.LipSyncPipeline.run_batch).parameters
    model = object()
    with pytest.raises(ValueError, match="up_face"):
        P.LipSyncPipeline(None, None, device="cpu", up_face=model, up_face_name="happy")
    with pytest.raises(ValueError, match="up_face"):
        P.LipSyncPipeline(None, None, device="cpu", up_face=model)
    with pytest.raises(ValueError, match="needs the GANimation model"):
        P.LipSyncPipeline(None, None, device="cpu", up_face_name="sad")
    pipe = P.LipSyncPipeline(None, None, device="cpu", batch=3, up_face=model, up_face_name="angry", without_rl1=True)
    assert tuple(pipe._aus.shape) == (3, 17) and torch.equal(pipe._aus[2], torch.tensor([0, 0, 0.3] + [0] * 14))
    mel, src, coeff = torch.zeros(2, 1, 80, 16), torch.zeros(2, 3, 256, 256), torch.zeros(2, 73, 26)
    with pytest.raises(ValueError, match="orig_u8"):                      # required with without_rl1
        pipe.run(mel, src, coeff)
    with pytest.raises(ValueError, match="orig_u8"):
        pipe.run(mel, src, coeff, orig_u8=torch.zeros(2, 384, 384, 3))    # not uint8
    with pytest.raises(ValueError, match="orig_u8"):
        pipe.run(mel, src, coeff, orig_u8=torch.zeros(2, 256, 256, 3, dtype=torch.uint8))
    with pytest.raises(ValueError, match="orig_u8"):
        pipe.run_batch(mel, src, coeff, torch.zeros(2, 3, 384, 384, dtype=torch.uint8))


def test_entry_points_reject_bad_arguments():
    from s2v_amd import _lib
    lib = _lib.load()
    p = lambda a: a.ctypes.data  # noqa: E731
    u8 = np.zeros(8 * 8 * 3, np.uint8)
    f = np.zeros(4096, np.float32)
    g = np.zeros(4096, np.float32)
    assert f.ctypes.data % 16 == 0 and g.ctypes.data % 16 == 0
    aus = np.zeros(34, np.float32)
    # gani_input: null pointers, empty sizes, a row pitch below the row, a misaligned output
    assert lib.s2v_gani_input(None, 1, 8, 8, 24, 192, p(aus), p(f), 4, 4, None) == -1
    assert lib.s2v_gani_input(p(u8), 1, 8, 8, 24, 192, None, p(f), 4, 4, None) == -1
    assert lib.s2v_gani_input(p(u8), 1, 8, 8, 24, 192, p(aus), None, 4, 4, None) == -1
    assert lib.s2v_gani_input(p(u8), 0, 8, 8, 24, 192, p(aus), p(f), 4, 4, None) == -1
    assert lib.s2v_gani_input(p(u8), 1, 8, 8, 24, 192, p(aus), p(f), 0, 4, None) == -1
    assert lib.s2v_gani_input(p(u8), 1, 8, 8, 23, 192, p(aus), p(f), 4, 4, None) == -1
    assert b"pitches" in lib.s2v_last_error()
    assert lib.s2v_gani_input(p(u8), 2, 4, 8, 24, 95, p(aus), p(f), 4, 4, None) == -1
    assert lib.s2v_gani_input(p(u8), 1, 8, 8, 24, 192, p(aus), p(f) + 4, 4, 4, None) == -1
    assert b"aligned" in lib.s2v_last_error()
    # gani_blend: null pointers, pitches off the multiple of 4 or below 4, misaligned inputs
    for bad in ((None, 4, p(g), 20), (p(f), 4, None, 20), (p(f), 3, p(g), 20), (p(f), 4, p(g), 18), (p(f), 4, p(g), 0),
                (p(f) + 4, 4, p(g), 20)):
        assert lib.s2v_gani_blend(bad[0], bad[1], bad[2], bad[3], 1, 4, 4, p(f), p(f), p(f), None) == -1
    assert lib.s2v_gani_blend(p(f), 4, p(g), 20, 1, 4, 4, None, p(f), p(f), None) == -1
    assert lib.s2v_gani_blend(p(f), 4, p(g), 20, 1, 0, 4, p(f), p(f), p(f), None) == -1
    # gani_compose: null pointers, an output mode other than 0 / 1, an empty fake, short pitches
    assert lib.s2v_gani_compose(None, p(u8), 24, 192, p(g), 4, 4, 1, 8, 8, p(f), 0, None) == -1
    assert lib.s2v_gani_compose(p(f), None, 24, 192, p(g), 4, 4, 1, 8, 8, p(f), 0, None) == -1
    assert lib.s2v_gani_compose(p(f), p(u8), 24, 192, p(g), 4, 4, 1, 8, 8, None, 0, None) == -1
    assert lib.s2v_gani_compose(p(f), p(u8), 24, 192, p(g), 4, 4, 1, 8, 8, p(f), 2, None) == -1
    assert lib.s2v_gani_compose(p(f), p(u8), 24, 192, p(g), 0, 4, 1, 8, 8, p(f), 0, None) == -1
    assert b"fake_img" in lib.s2v_last_error()
    assert lib.s2v_gani_compose(p(f), p(u8), 23, 192, None, 0, 0, 1, 8, 8, p(f), 0, None) == -1
    assert lib.s2v_gani_compose(p(f), p(u8), 24, 191, None, 0, 0, 2, 8, 8, p(f), 0, None) == -1
    assert lib.s2v_gani_compose(p(f), p(u8), 24, 192, None, 0, 0, 1, 8, 8, p(f) + 2, 0, None) == -1


# ----------------------------------------------------------------------------- the restatements
def test_restatement_of_lines_277_286_equals_the_fixture_probes(golden):
    """The fixture stores probes of every stage of lines 277-286, not whole tensors, so the generator runs here
    again: layer for layer in torch on the CPU from the mirror's state_dict alone.  That pins the architecture
    the engine implements (biases, IN eps, where the residual enters) to the reference's recorded outputs, and
    then the restatement of the composite (tests/ganimation_cases.py) to its recorded frames."""
    g = golden("ganimation_goldens_128")
    sdict = GC.state_dict()

    def inorm(t):
        return F.instance_norm(t, eps=1e-5)

    def net(img, aus):
        x = torch.cat([img, aus[:, :, None, None].expand(-1, -1, *img.shape[2:])], 1)
        w = lambda k: (sdict[k + ".weight"], sdict[k + ".bias"])  # noqa: E731
        h = F.relu(inorm(F.conv2d(x, *w("model.0"), padding=3)))
        for i in (3, 6):
            h = F.relu(inorm(F.conv2d(h, *w(f"model.{i}"), stride=2, padding=1)))
        for i in range(9, 15):
            t = F.relu(inorm(F.conv2d(h, *w(f"model.{i}.conv_block.0"), padding=1)))
            h = h + inorm(F.conv2d(t, *w(f"model.{i}.conv_block.3"), padding=1))
        for i in (15, 18):
            h = F.relu(inorm(F.conv_transpose2d(h, *w(f"model.{i}"), stride=2, padding=1)))
        return (torch.tanh(F.conv2d(h, sdict["color_top.0.weight"], padding=3)),
                torch.sigmoid(F.conv2d(h, sdict["au_top.0.weight"], padding=3)), h)

    pred, orig = GC.compose_inputs()
    _, aus = GC.net_inputs(GC.COMPOSE_CASE)
    src = GC.src128(orig)
    assert torch.equal(torch.from_numpy(g["compose_src_probe"]), torch.from_numpy(GC.probe(src, "ganimation.src")))
    torch.set_num_threads(min(8, os.cpu_count() or 1))
    with torch.no_grad():
        color, a, _ = net(src, aus[:1].repeat(len(orig), 1))
    fake = a * src + (1 - a) * color
    # the same network in another summation order: fp32 rounding only
    assert np.abs(GC.probe(fake, "ganimation.fake") - g["compose_fake_probe"]).max() < 1e-4
    out, out_u8 = GC.compose_ref(pred, orig, fake)
    d = np.abs(GC.probe(out, "ganimation.out") - g["compose_out_probe"])
    assert d.max() < 1e-4
    du = np.abs(GC.probe(out_u8, "ganimation.out").astype(int) - g["compose_u8_probe"].astype(int))
    assert du.max() <= 1 and (du == 0).mean() > 0.99
    # up_face == 'original' needs no network: exact
    plain, plain_u8 = GC.compose_ref(pred, orig, None)
    assert np.array_equal(GC.probe(plain, "ganimation.out"), g["compose_plain_probe"])
    assert np.array_equal(GC.probe(plain_u8, "ganimation.out"), g["compose_plain_u8_probe"])
    # the composite keeps the prediction in the lower half and takes the originals' place only above it
    pc = torch.clamp(pred, 0, 1)
    P = GC.COMPOSE_P
    assert torch.equal(out[:, :, P // 2:], pc[:, :, P // 2:])
    zero = torch.from_numpy(orig.transpose(0, 3, 1, 2) == 0)
    assert zero[:, :, : P // 2].any() and not zero[:, :, P // 2:].any()
    assert torch.equal(out[zero], pc[zero]) and (out[:, :, : P // 2][~zero[:, :, : P // 2]] !=
                                                 pc[:, :, : P // 2][~zero[:, :, : P // 2]]).float().mean() > 0.99
    # float64 agrees with the fp32 evaluation to the rounding of fp32 source coordinates: an ulp of 7.6e-6 at
    # coordinate 127, times a neighbour difference below 1
    out64, _ = GC.compose_ref(pred, orig, fake, torch.float64)
    assert (out64 - out.double()).abs().max() < 1e-5


def test_restatements_of_input_and_blend():
    u8 = GC.image_u8("host.in", 2, 384, 384)
    aus = np.linspace(0, 1, 34, dtype=np.float32).reshape(2, 17)
    x = GC.input_ref(u8, aus)
    assert x.shape == (2, 128, 128, 20)
    # 384 -> 128: source index 3 i + 1 with weights 1 and 0
    want = torch.from_numpy(u8[:, 1::3, 1::3]).float() / 255. * 2 - 1
    assert torch.equal(x[..., :3], want)
    assert torch.equal(x[..., 3:], torch.from_numpy(aus)[:, None, None, :].expand(2, 128, 128, 17))
    head = torch.tensor([[[[0.0]], [[12.0]], [[-12.0]], [[0.0]]]])
    src = torch.full((1, 3, 1, 1), 0.5)
    color, a, fake = GC.blend_ref(head, src)
    assert a.item() == 0.5 and color[0, 0].item() == 0 and abs(color[0, 1].item() - 1) < 1e-9
    assert torch.allclose(fake.flatten(), torch.tensor([0.25, 0.75, -0.25], dtype=torch.float64), atol=1e-9)
