"""GANimation upper-face editing on the device: the three kernels of csrc/gani.hip against their restatements
(tests/ganimation_cases.py: torch on the CPU, fp64 for the transcendentals), the engine and GANimationModel
against tests/golden/ganimation_goldens*.npz (recorded from the reference's SplitGenerator by
tests/golden/make_ganimation_golden.py), the ``up_face`` / ``without_rl1`` stage of LipSyncPipeline and
inference.run(up_face=..., without_rl1=True).

Bars:
* s2v_gani_input: the action-unit channels exactly; 384 -> 128 bit-exact (source index 3 i + 1, weights 1 and
  0); other sizes atol 5e-7 (lerps of values in [-1, 1]: the restatement's builds may fuse a product);
* s2v_gani_blend: atol 2e-6 against fp64 (outputs bounded by 1, a few ulp per transcendental, three combined);
* s2v_gani_compose: float atol 1e-6 against the restatement, the uint8 output exactly trunc(255 * float output);
* forward: logits and embed probes within eps = 1e-3 * max(1, max|ref|); color_mask within eps (tanh' <= 1),
  aus_mask within eps / 4 (sigmoid' <= 1/4), fake_img within 1.5 eps (|da| * |src - color| <= 2 eps / 4, plus eps).
"""
import numpy as np
import pytest
import torch

import s2v_import  # noqa: F401
import ganimation_cases as GC
from helpers import synth_sd, write_mp4_header, write_wav
from s2v_amd import synth

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _dev(a):
    if isinstance(a, torch.Tensor):
        return a.contiguous().to(DEV)
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


@pytest.fixture(scope="module")
def ctx():
    from s2v_amd import ops
    return ops.Ctx(torch.device(DEV, torch.cuda.current_device()))


@pytest.fixture(scope="module")
def G(golden):
    g = {}
    for name in ("ganimation_goldens", "ganimation_goldens_128", "ganimation_goldens_128_masks"):
        g.update(golden(name))
    return g


@pytest.fixture(scope="module")
def net_gen():
    from s2v_amd import models
    net = models.SplitGenerator()
    net.load_state_dict(GC.state_dict(), strict=True)
    return net.eval()


@pytest.fixture(scope="module")
def model(net_gen):
    from s2v_amd import ganimation
    return ganimation.GANimationModel().initialize(net_gen=net_gen, device=DEV).setup()


# ----------------------------------------------------------------------------- s2v_gani_input
@pytest.mark.parametrize("P,Q,oh,ow", [(384, 384, 128, 128), (256, 256, 128, 128), (100, 100, 128, 128), (20, 30, 8, 12)])
def test_gani_input_matches_interpolate(ctx, P, Q, oh, ow):
    from s2v_amd import ganimation
    n = 2
    u8 = GC.image_u8(f"in{P}x{Q}", n, P, Q)
    aus = synth.hash_array(f"ganimation.in{P}.aus", (n, 17), 0.0, 1.0)
    got = ganimation.gani_input(ctx, _dev(u8), _dev(aus), (oh, ow)).t.cpu()
    ref = GC.input_ref(u8, aus, (oh, ow))
    assert got.shape == (n, oh, ow, 20)
    assert torch.equal(got[..., 3:], ref[..., 3:])                                     # the action units, exactly
    d = (got[..., :3] - ref[..., :3]).abs().max().item()
    print(f"gani_input {P}x{Q} -> {oh}x{ow}: max |d| {d:.3e}")
    if (P, Q) == (384, 384):
        assert torch.equal(got, ref)
    else:
        assert d <= 5e-7


def test_gani_input_wide_pitch_and_output_bounds(ctx):
    """Originals as a view into a larger buffer (row pitch wider than the row, rows above and below): the
    padding is never read into the result, and nothing is written past the output."""
    from s2v_amd._lib import check
    n, P, Q, oh, ow = 2, 20, 30, 8, 12
    u8 = GC.image_u8("pitch", n, P, Q)
    aus = _dev(synth.hash_array("ganimation.pitch.aus", (n, 17), 0.0, 1.0))
    outs = []
    for fill in (0, 255):
        big = torch.full((n, P + 3, Q * 3 + 7), fill, dtype=torch.uint8, device=DEV)
        view = big[:, 2:2 + P, 5:5 + Q * 3].unflatten(2, (Q, 3))
        view.copy_(_dev(u8))
        total = n * oh * ow * 20
        flat = torch.full((total + 64,), 7.0, device=DEV)
        check(ctx.lib.s2v_gani_input(view.data_ptr(), n, P, Q, view.stride(1), view.stride(0), aus.data_ptr(),
                                     flat.data_ptr(), oh, ow, ctx.stream), "s2v_gani_input")
        assert torch.equal(flat[total:].cpu(), torch.full((64,), 7.0))
        outs.append(flat[:total].view(n, oh, ow, 20).cpu())
    assert torch.equal(outs[0], outs[1])
    assert (outs[0] - GC.input_ref(u8, aus.cpu(), (oh, ow))).abs().max() <= 5e-7


# ----------------------------------------------------------------------------- s2v_gani_blend
@pytest.mark.parametrize("h,w", [(5, 7), (32, 32)])
def test_gani_blend_matches_fp64(ctx, h, w):
    from s2v_amd import models, ops
    n = 2
    head = synth.hash_array(f"ganimation.blend{h}.head", (n, h, w, 4), -12.0, 12.0)
    head[0, 0, 0] = (12.0, -12.0, 0.0, 12.0)                                         # both rails and the centre
    head[0, 0, 1] = (0.0, 1e-4, -1e-4, -12.0)
    x20 = synth.hash_array(f"ganimation.blend{h}.in", (n, h, w, 20), -1.0, 1.0)
    color, a, fake = models.SplitGenerator.blend(ctx, ops.NHWC(_dev(head)), ops.NHWC(_dev(x20)))
    assert color.shape == (n, 3, h, w) and a.shape == (n, 1, h, w) and fake.shape == (n, 3, h, w)
    rc, ra, rf = GC.blend_ref(torch.from_numpy(head).permute(0, 3, 1, 2), torch.from_numpy(x20[..., :3]).permute(0, 3, 1, 2))
    errs = [(g.cpu().double() - r).abs().max().item() for g, r in ((color, rc), (a, ra), (fake, rf))]
    print(f"gani_blend {h}x{w}: max |d| color {errs[0]:.2e} mask {errs[1]:.2e} fake {errs[2]:.2e}")
    assert max(errs) <= 2e-6


# ----------------------------------------------------------------------------- s2v_gani_compose
def _compose_both(ctx, pred, orig, fake, off_u8=0, off_f=0):
    """The kernel's float and uint8 outputs inside guarded buffers (``off``: elements the output starts past
    the buffer's aligned base, after 16 guard elements)."""
    from s2v_amd import ganimation
    n, _, ph, pw = pred.shape
    total = n * 3 * ph * pw
    pd, od = _dev(pred), _dev(orig)
    fd = None if fake is None else _dev(fake)
    fbuf = torch.full((total + 48,), -3.0, device=DEV)
    ubuf = torch.full((total + 48,), 201, dtype=torch.uint8, device=DEV)
    f0, u0 = 16 + off_f, 16 + off_u8
    ganimation.gani_compose(ctx, pd, od, fd, fbuf[f0:f0 + total].view(n, 3, ph, pw))
    ganimation.gani_compose(ctx, pd, od, fd, ubuf[u0:u0 + total].view(n, 3, ph, pw))
    fb, ub = fbuf.cpu(), ubuf.cpu()
    assert (fb[:f0] == -3.0).all() and (fb[f0 + total:] == -3.0).all()               # nothing outside the output
    assert (ub[:u0] == 201).all() and (ub[u0 + total:] == 201).all()
    return fb[f0:f0 + total].view(n, 3, ph, pw), ub[u0:u0 + total].view(n, 3, ph, pw)


@pytest.mark.parametrize("fh,fw,ph,pw,off", [(8, 8, 24, 24, 0), (8, 8, 24, 24, 1), (5, 7, 12, 18, 0), (5, 7, 12, 18, 1),
                                             (4, 4, 9, 13, 0), (4, 4, 9, 13, 1), (128, 128, 384, 384, 0),
                                             (0, 0, 24, 24, 0), (0, 0, 12, 18, 1)])
def test_gani_compose_matches_restatement(ctx, fh, fw, ph, pw, off):
    """fh == 0: fake NULL (up_face 'original').  Widths 18 and 13 leave a ragged row end and rows off the
    dword alignment; ``off`` 1 moves the output's base off it too (byte and scalar stores)."""
    n = 2
    key = f"cmp{fh}x{fw}.{ph}x{pw}"
    pred, orig = GC.pred_values(key, n, ph, pw), GC.originals(key, n, ph, pw)
    fake = torch.from_numpy(synth.hash_array(f"ganimation.{key}.fake", (n, 3, fh, fw), -1.0, 1.0)) if fh else None
    got_f, got_u8 = _compose_both(ctx, pred, orig, fake, off_u8=off, off_f=off)
    ref_f, ref_u8 = GC.compose_ref(pred, orig, fake)
    d = (got_f - ref_f).abs().max().item()
    flips = int((got_u8 != torch.from_numpy(ref_u8)).sum())
    print(f"gani_compose {key} off {off}: max |d| {d:.3e}, {flips} uint8 values differ from the restatement's")
    assert pred.min() < 0 and pred.max() > 1 and (orig[:, : ph // 2] == 0).any() and (orig[:, ph // 2:] != 0).all()
    assert d <= 1e-6
    # the uint8 mode is the truncation of the float mode, bit for bit
    assert torch.equal(got_u8, torch.from_numpy((got_f.numpy() * 255.).astype(np.uint8)))
    # where the mask keeps the prediction the value is the clamped prediction itself
    keep = torch.from_numpy(orig.transpose(0, 3, 1, 2) == 0)
    keep[:, :, ph // 2:] = True
    assert torch.equal(got_f[keep], pred.clamp(0, 1)[keep])
    if fake is None:
        assert torch.equal(got_f, ref_f) and flips == 0                               # no interpolation: exact


# ----------------------------------------------------------------------------- engine forward
def _x20(img, aus):
    x = torch.cat([img, aus[:, :, None, None].expand(-1, -1, *img.shape[2:])], 1)
    return _dev(x.permute(0, 2, 3, 1))


@pytest.mark.parametrize("case", list(GC.CASES))
def test_forward_matches_reference(G, net_gen, prec, case):
    from s2v_amd import ops
    img, aus = GC.net_inputs(case)
    x20 = ops.NHWC(_x20(img, aus))
    (head, embed), ctx = net_gen.forward_nhwc(x20)
    color, a, fake = net_gen.blend(ctx, head, x20)
    ref = G[f"{case}_logits"]
    eps = GC.forward_eps(np.abs(ref).max())
    eps_e = GC.forward_eps(G[f"{case}_embed_max"])
    got_logits = head.t.permute(0, 3, 1, 2).cpu().numpy()
    got_embed = GC.probe(embed.t.permute(0, 3, 1, 2).contiguous(), "ganimation.embed")
    errs = {"logits": np.abs(got_logits - ref).max(), "embed": np.abs(got_embed - G[f"{case}_embed_probe"]).max(),
            "color": np.abs(color.cpu().numpy() - G[f"{case}_color_mask"]).max(),
            "aus": np.abs(a.cpu().numpy() - G[f"{case}_aus_mask"]).max(),
            "fake": np.abs(fake.cpu().numpy() - G[f"{case}_fake_img"]).max()}
    print(f"forward {case} {prec}: eps {eps:.2e} / embed {eps_e:.2e}; " + ", ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    assert errs["logits"] <= eps and errs["embed"] <= eps_e
    assert errs["color"] <= eps and errs["aus"] <= eps / 4 and errs["fake"] <= 1.5 * eps


def test_forward_rejects_sizes_off_the_multiple_of_4(net_gen):
    from s2v_amd import ops
    for hw in ((30, 32), (32, 34)):
        with pytest.raises(ValueError, match="multiples of 4"):
            net_gen.forward_nhwc(ops.NHWC(torch.zeros((1, *hw, 20), device=DEV)))


def test_split_generator_forward_is_the_references_triple(G, net_gen):
    img, aus = GC.net_inputs("b2_32")
    color, a, embed = net_gen(_dev(img), _dev(aus))
    eps = GC.forward_eps(np.abs(G["b2_32_logits"]).max())
    assert embed.shape == (2, 64, 32, 32)
    assert np.abs(color.cpu().numpy() - G["b2_32_color_mask"]).max() <= eps
    assert np.abs(a.cpu().numpy() - G["b2_32_aus_mask"]).max() <= eps / 4
    assert np.abs(GC.probe(embed, "ganimation.embed") - G["b2_32_embed_probe"]).max() <= GC.forward_eps(G["b2_32_embed_max"])


# ----------------------------------------------------------------------------- GANimationModel
def test_model_attributes_and_lines_277_286(G, model, ctx):
    from s2v_amd import ganimation
    case = GC.COMPOSE_CASE
    img, aus = GC.net_inputs(case)
    model.feed_batch({"src_img": img, "tar_aus": aus})
    model.forward()
    eps = GC.forward_eps(np.abs(G[f"{case}_logits"]).max())
    errs = [np.abs(getattr(model, k).cpu().numpy() - G[f"{case}_{k}"]).max() for k in ("color_mask", "aus_mask", "fake_img")]
    e_embed = np.abs(GC.probe(model.embed, "ganimation.embed") - G[f"{case}_embed_probe"]).max()
    print(f"model {case}: eps {eps:.2e}; color {errs[0]:.2e} aus {errs[1]:.2e} fake {errs[2]:.2e} embed {e_embed:.2e}")
    assert errs[0] <= eps and errs[1] <= eps / 4 and errs[2] <= 1.5 * eps
    assert model.embed.shape == (2, 64, 128, 128) and e_embed <= GC.forward_eps(G[f"{case}_embed_max"])
    # inference.py:277-286 from the uint8 originals: resize, generator, blend, resize back, composite
    pred, orig = GC.compose_inputs()
    tar = _dev(aus[:1].repeat(len(orig), 1))
    fake = model.edit(_dev(orig), tar)
    assert fake is model.fake_img and fake.shape == (2, 3, 128, 128)
    e_fake = np.abs(GC.probe(fake, "ganimation.fake") - G["compose_fake_probe"]).max()
    out = torch.empty((2, 3, GC.COMPOSE_P, GC.COMPOSE_P), device=DEV)
    ganimation.gani_compose(ctx, _dev(pred), _dev(orig), fake, out)
    out_u8 = torch.empty(out.shape, dtype=torch.uint8, device=DEV)
    ganimation.gani_compose(ctx, _dev(pred), _dev(orig), fake, out_u8)
    # eps at its floor of 1e-3 (frames lie in [0, 1]): the edit enters the frame halved (fake / 2 + 0.5)
    bar = 1.5 * 1e-3 / 2 + 1e-6
    e_out = np.abs(GC.probe(out, "ganimation.out") - G["compose_out_probe"]).max()
    du = np.abs(GC.probe(out_u8, "ganimation.out").astype(int) - G["compose_u8_probe"].astype(int))
    print(f"lines 277-286: fake {e_fake:.2e}, frames {e_out:.2e} (bar {bar:.2e}), uint8 probes off by one: {int((du > 0).sum())}"
          f" of {du.size}")
    assert e_fake <= 1.5 * 1e-3 and e_out <= bar
    assert du.max() <= 1 and (du == 0).mean() >= 0.99                  # bar * 255 = 0.19 of a level
    # up_face == 'original': the unedited crops, exact
    plain = torch.empty_like(out)
    ganimation.gani_compose(ctx, _dev(pred), _dev(orig), None, plain)
    assert np.array_equal(GC.probe(plain, "ganimation.out"), G["compose_plain_probe"])


# ----------------------------------------------------------------------------- pipeline and runner
@pytest.fixture(scope="module")
def nets_pair():
    from s2v_amd import models
    d = models.DNet()
    d.load_state_dict(synth_sd("dnet"), strict=True)
    e = models.ENet()
    e.load_state_dict(synth_sd("enet"), strict=True)                   # StyleConv noise weights 0: noise off
    return d.eval(), e.eval()


def test_pipeline_up_face_and_without_rl1(nets_pair, model, monkeypatch):
    from s2v_amd import ops
    from s2v_amd import pipeline as P
    dnet, enet = nets_pair
    b = 2
    src, coeff = synth.dnet_inputs("ganimation.pipeline", b, 256)
    src, coeff = _dev(src), _dev(coeff)
    mel = _dev(synth.hash_array("ganimation.pipeline.mel", (b, 1, 80, 16), -4.0, 4.0))
    orig = GC.originals("pipeline", b, 384, 384)
    orig_d = _dev(orig)
    calls = []
    edit = model.edit
    monkeypatch.setattr(model, "edit", lambda *a, **k: (calls.append(1), edit(*a, **k))[1])

    def run(**kw):
        pipe = P.LipSyncPipeline(dnet, enet, device=DEV, batch=b, graph=False, **kw)
        out = torch.empty((b, 3, 384, 384), dtype=torch.uint8, device=DEV)
        pipe.run_batch(mel, src, coeff, out, 0, *((orig_d,) if kw.get("without_rl1") else ()))
        return out.clone()

    plain = run()
    # up_face alone: the reference drops the edit; no generator forward, the frames bit-identical
    assert torch.equal(run(up_face=model, up_face_name="sad"), plain) and not calls
    edited = run(up_face=model, up_face_name="surprise", without_rl1=True)
    assert len(calls) == 1
    fake = model.fake_img.clone()
    # the pipeline's own prediction, by the launches run_batch makes
    with torch.no_grad():
        dn = dnet(src, coeff, lane=0)["fake_image"]
        ref_u8 = torch.empty((b, 3, 256, 256), dtype=torch.uint8, device=DEV)
        face6 = torch.empty((b, 6, 256, 256), device=DEV)
        gt = torch.empty((b, 3, 256, 256), device=DEV)
        ops.S2V.lipsync_inputs_(src.contiguous(), dn, ref_u8, face6, gt)
        pred, _ = enet(mel, face6, gt, lane=0)
        today = torch.empty((b, 3, 384, 384), dtype=torch.uint8, device=DEV)
        ops.S2V.to_u8_(pred, today, 0.0, 1.0, 255.0, 0.0)
    assert torch.equal(plain, today)
    _, want = GC.compose_ref(pred.cpu(), orig, fake.cpu())
    want = torch.from_numpy(want)
    d = (edited.cpu().int() - want.int()).abs()
    keep = torch.from_numpy(orig.transpose(0, 3, 1, 2) == 0)
    keep[:, :, 192:] = True
    print(f"pipeline: {int((d > 0).sum())} of {d.numel()} uint8 values differ from the restatement (max {int(d.max())})")
    # the float frames agree to 1e-6 (test_gani_compose_matches_restatement), so a level can flip only where
    # 255 v sits within 2.6e-4 of an integer
    assert d.max() <= 1 and (d == 0).float().mean() >= 0.999
    assert torch.equal(edited.cpu()[keep], plain.cpu()[keep]) and torch.equal(edited.cpu()[keep], want[keep])
    assert (edited.cpu()[~keep] != plain.cpu()[~keep]).float().mean() > 0.9
    # without_rl1 alone composites the unedited crops: exact
    only = run(without_rl1=True)
    assert torch.equal(only.cpu(), torch.from_numpy(GC.compose_ref(pred.cpu(), orig, None)[1])) and len(calls) == 1
    # the stage has no host step: full batches replay captured graphs, bit for bit the eager frames
    pipe = P.LipSyncPipeline(dnet, enet, device=DEV, batch=b, graph=True, up_face=model, up_face_name="surprise",
                             without_rl1=True)
    first = pipe.run(mel, src, coeff, orig_u8=orig_d)
    again = pipe.run(mel, src, coeff, orig_u8=orig_d)
    assert pipe._runner is not None and pipe._runner.k == 2
    assert torch.equal(first, edited) and torch.equal(again, edited)


def test_runner_up_face(tmp_path):
    from s2v_amd import inference
    face = str(write_mp4_header(tmp_path / "v.mp4", 128, 96, 12, 12800, 6144))          # 25 fps
    wav = str(write_wav(tmp_path / "a.wav", rate=16000, channels=1, seconds=0.5))
    r = inference.run(face, wav, max_frames=4, batch=4, up_face="surprise", without_rl1=True)
    m = r["meta"]
    assert (m["up_face"], m["without_rl1"], m["up_face_weights"]) == ("surprise", True, "30_net_gen synthetic")
    plain = inference.run(face, wav, max_frames=4, batch=4)
    pm = plain["meta"]
    assert (pm["up_face"], pm["without_rl1"], pm["up_face_weights"]) == ("original", False, None)
    a, b = r["preds"], plain["preds"]
    assert a.shape == b.shape == (4, 3, 384, 384)
    assert torch.equal(a[:, :, 192:], b[:, :, 192:])                     # the lower half is the prediction's
    assert (a[:, :, :192] != b[:, :, :192]).float().mean() > 0.9         # the upper half is the edited crop's
    with pytest.raises(ValueError, match="up_face"):
        inference.run(face, wav, max_frames=4, batch=4, up_face="happy")
