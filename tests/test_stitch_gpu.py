"""The reference stitch on the device: the two kernels of csrc/stitch.hip and s2v_amd.stitch against
tests/golden/stitch_goldens.npz (recorded from the reference's futils/alignment_stit.py and Pillow by
tests/golden/make_stitch_golden.py), the ``stitch`` stage of LipSyncPipeline and inference.run(stitch=True).

Bars:
* s2v_pil_transform_quad and s2v_pil_perspective_paste: BIT-EXACT on every golden case, coefficients taken from
  the fixture (so the host's LAPACK cannot enter), in 3- and 4-channel layouts, with strided inputs and outputs
  (both the dword and the byte store path) and pasting in place;
* crop_faces / paste_image / Stitcher: BIT-EXACT on their cases with the coefficients our host code computes;
* the pipeline stage equals a ref_hook that applies the Stitcher by hand, changes the output, and leaves the
  output without it exactly what the sequence of launches gave before.
"""
import numpy as np
import pytest
import torch

import s2v_import  # noqa: F401
import stitch_cases as SC
from helpers import write_mp4_header, write_wav

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module")
def G(golden):
    return golden("stitch_goldens")


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _table(G, name):
    box = G[f"quad.{name}.box"].astype(np.float64)
    return np.concatenate([G[f"quad.{name}.coef"], [box[0], box[1], box[2] - box[0], box[3] - box[1]]])[None]


def _frame(name):
    W, H, _, _ = SC.QUAD_CASES[name]
    return SC.image(name, H, W)


# ----------------------------------------------------------------------------- s2v_pil_transform_quad
@pytest.mark.parametrize("name", list(SC.QUAD_CASES))
def test_transform_quad_bit_exact(G, name):
    from s2v_amd import stitch as ST
    S = SC.QUAD_CASES[name][2]
    got = ST.transform_quad(_dev(_frame(name)), _table(G, name), S)[0].cpu().numpy()
    ref = G[f"quad.{name}.crop"]
    print(f"{name}: {int((got != ref).sum())} bytes differ, zero pixels {(ref.sum(2) == 0).mean():.2f}")
    assert np.array_equal(got, ref)


def test_transform_quad_batch_of_four_in_one_launch(G):
    from s2v_amd import stitch as ST
    frames = _dev(np.stack([_frame(n) for n in SC.SMALL]))
    table = np.concatenate([_table(G, n) for n in SC.SMALL])
    got = ST.transform_quad(frames, table, 32).cpu().numpy()
    for i, n in enumerate(SC.SMALL):
        assert np.array_equal(got[i], G[f"quad.{n}.crop"]), n


@pytest.mark.parametrize("pad", [1, 4])
def test_transform_quad_four_channels_and_strides(G, pad):
    """RGBA frames inside a larger buffer, output rows inside a larger buffer: pad 1 breaks the 4-byte alignment
    of the 3-channel rows (byte stores), pad 4 keeps it (dword stores); nothing outside the views is written."""
    from s2v_amd import stitch as ST
    names = SC.SMALL
    rgb = np.stack([_frame(n) for n in names])
    a = np.stack([SC.image(f"{n}.band4", 40, 48, 1) for n in names])
    table = np.concatenate([_table(G, n) for n in names])
    for c, frames in ((3, rgb), (4, np.concatenate([rgb, a], 3))):
        big = torch.full((4, 40 + 3, 48 * c + 7), 201, dtype=torch.uint8, device=DEV)
        view = big[:, 2:42, 5:5 + 48 * c].unflatten(2, (48, c))
        view.copy_(_dev(frames))
        obig = torch.full((4, 32 + 2, 32 * c + pad), 77, dtype=torch.uint8, device=DEV)
        out = obig[:, 1:33, :32 * c].unflatten(2, (32, c))
        ST.transform_quad(view, table, 32, out=out)
        got = obig.cpu().numpy()
        assert (got[:, 0] == 77).all() and (got[:, 33] == 77).all() and (got[:, :, 32 * c:] == 77).all()
        got = got[:, 1:33, :32 * c].reshape(4, 32, 32, c)
        for i, n in enumerate(names):
            assert np.array_equal(got[i, :, :, :3], G[f"quad.{n}.crop"]), (n, c, pad)
            if c == 4:          # the fourth band against the NumPy restatement of Pillow's rule
                l, t, r, b = (int(v) for v in G[f"quad.{n}.box"])
                ref4 = SC.pil_quad(frames[i, t:b, l:r, 3:], G[f"quad.{n}.coef"], 32)
                assert np.array_equal(got[i, :, :, 3:], ref4), n


@pytest.mark.parametrize("pitch", [783, 784])
def test_transform_quad_ragged_width(pitch):
    """An output width that is no multiple of the four pixels a thread owns, more than one block per row: with
    the packed pitch 783 every thread stores bytes, with 784 the rows are 4-byte aligned and only the ragged last
    thread of a row does."""
    from s2v_amd import _lib, post
    W, H, S, quad = SC.QUAD_CASES["deep256"]
    frame = _frame("deep256")
    ow, oh = 261, 7
    l, t, r, b = 68, 58, 192, 182
    a = np.array([3.25, 0.41, 0.07, 1e-4, 2.5, -0.03, 0.9, 2e-4])
    table = np.concatenate([a, [l, t, r - l, b - t]])[None]
    out = torch.full((oh, pitch), 77, dtype=torch.uint8, device=DEV)
    ctx = post._ctx(torch.device(DEV))
    x, tab = _dev(frame), _dev(table)
    _lib.check(ctx.lib.s2v_pil_transform_quad(x.data_ptr(), 1, H, W, 3, W * 3, H * W * 3, tab.data_ptr(), out.data_ptr(),
                                              oh, ow, pitch, oh * pitch, ctx.stream), "s2v_pil_transform_quad")
    xx = np.arange(ow)[None, :] + 0.5
    yy = np.arange(oh)[:, None] + 0.5
    xin = a[0] + a[1] * xx + a[2] * yy + a[3] * xx * yy
    yin = a[4] + a[5] * xx + a[6] * yy + a[7] * xx * yy
    ref = SC.pil_bilinear(frame[t:b, l:r], xin, yin)
    got = out.cpu().numpy()
    assert (got[:, ow * 3:] == 77).all()
    assert np.array_equal(got[:, :ow * 3].reshape(oh, ow, 3), ref) and (ref.sum(2) == 0).any() and (ref.sum(2) > 0).any()


# ----------------------------------------------------------------------------- s2v_pil_perspective_paste
def _paste_case(G, name):
    """(crop, target, golden coefficients, golden output)."""
    if name in SC.QUAD_CASES:
        W, H, _, _ = SC.QUAD_CASES[name]
        crop = G[f"quad.{name}.crop"]
    else:
        W, H, S, ch, _ = SC.PASTE_CASES[name]
        crop = SC.image(f"{name}.crop", S, S, ch)
    return crop, SC.image(f"{name}.target", H, W), G[f"paste.{name}.coef"], G[f"paste.{name}.out"]


@pytest.mark.parametrize("name", list(SC.QUAD_CASES) + list(SC.PASTE_CASES))
def test_perspective_paste_bit_exact(G, name):
    from s2v_amd import stitch as ST
    crop, target, coef, ref = _paste_case(G, name)
    t = _dev(target)
    got = ST.paste_images(coef[None], _dev(crop)[None], t[None])[0].cpu().numpy()
    changed = (ref != target).any(2).mean()
    print(f"{name}: {int((got != ref).sum())} bytes differ, pasted share {changed:.2f}")
    assert np.array_equal(got, ref)
    assert np.array_equal(t.cpu().numpy(), target)                       # the target is only read
    if name == "miss":
        assert changed == 0
    if name in ("cover", "wide256"):
        assert changed > 0.98
    # in place: target and output are one buffer
    got = ST.paste_images(coef[None], _dev(crop)[None], t[None], out=t[None])[0].cpu().numpy()
    assert np.array_equal(got, ref)


@pytest.mark.parametrize("pad", [1, 4])
def test_perspective_paste_layouts_and_strides(G, pad):
    """A batch of four in one launch with RGBA targets, RGB and RGBA outputs, everything inside larger buffers
    (pad 1: byte stores, pad 4: dword stores); the 4-channel crop with alpha in 0..255 rides along."""
    from s2v_amd import stitch as ST
    names = ("inside", "topleft", "trapezoid", "cover")
    cases = [_paste_case(G, n) for n in names]
    coef = np.stack([c[2] for c in cases])
    crops = np.stack([c[0] for c in cases])
    targets = np.stack([c[1] for c in cases])
    cbig = torch.full((4, 33, 32 * 3 + 5), 9, dtype=torch.uint8, device=DEV)
    cview = cbig[:, 1:33, 2:2 + 96].unflatten(2, (32, 3))
    cview.copy_(_dev(crops))
    t4 = _dev(np.concatenate([targets, np.full((4, 40, 48, 1), 31, np.uint8)], 3))
    for oc in (3, 4):
        obig = torch.full((4, 42, 48 * oc + pad), 77, dtype=torch.uint8, device=DEV)
        out = obig[:, 1:41, :48 * oc].unflatten(2, (48, oc))
        ST.paste_images(coef, cview, t4, out=out)
        got = obig.cpu().numpy()
        assert (got[:, 0] == 77).all() and (got[:, 41] == 77).all() and (got[:, :, 48 * oc:] == 77).all()
        got = got[:, 1:41, :48 * oc].reshape(4, 40, 48, oc)
        for i, n in enumerate(names):
            assert np.array_equal(got[i, :, :, :3], cases[i][3]), (n, oc, pad)
        if oc == 4:
            assert (got[..., 3] == 255).all()
    # the RGBA crop (Pillow's premultiplied round trip and the general blend) next to an RGB-derived one
    crop, target, c, ref = _paste_case(G, "rgba")
    assert len(np.unique(crop[..., 3])) > 200
    got = ST.paste_images(np.stack([c, c]), _dev(np.stack([crop, crop])), _dev(np.stack([target, target])))
    assert np.array_equal(got[0].cpu().numpy(), ref) and np.array_equal(got[1].cpu().numpy(), ref)
    opaque = G["paste.trapezoid.out"]
    assert not np.array_equal(ref, opaque)


@pytest.mark.parametrize("pitch", [150, 152])
def test_perspective_paste_ragged_width(G, pitch):
    """A target 50 pixels wide (twelve threads of four and one of two) against the NumPy restatement of
    paste_image: packed rows (pitch 150, byte stores) and 4-byte-aligned rows (152: dwords, bytes for the ragged
    last thread), out of place and in place."""
    from s2v_amd import stitch as ST
    crop = SC.image("ragged.crop", 32, 32, 4)
    target = SC.image("ragged.target", 9, 50)
    coef = ST.calc_alignment_coefficients([[3.0, 1.0], [1.0, 8.0], [47.0, 7.5], [44.0, 0.5]], ST.square(32))
    ref = SC.pil_paste(crop, coef, target)
    assert 0.3 < (ref != target).any(2).mean() < 1.0
    tbig = torch.full((9, pitch), 55, dtype=torch.uint8, device=DEV)
    tview = tbig[:, :150].unflatten(1, (50, 3))
    tview.copy_(_dev(target))
    obig = torch.full((9, pitch), 77, dtype=torch.uint8, device=DEV)
    ST.paste_images(coef[None], _dev(crop)[None], tview[None], out=obig[:, :150].unflatten(1, (50, 3))[None])
    got = obig.cpu().numpy()
    assert np.array_equal(got[:, :150].reshape(9, 50, 3), ref) and (got[:, 150:] == 77).all()
    ST.paste_images(coef[None], _dev(crop)[None], tview[None], out=tview[None])
    got = tbig.cpu().numpy()
    assert np.array_equal(got[:, :150].reshape(9, 50, 3), ref) and (got[:, 150:] == 55).all()


def test_overlapping_buffers_are_rejected(G):
    """In place means the same pointer and layout; a shifted view of the target, or an output inside the crops
    or the frames, is refused before any launch."""
    from s2v_amd import _lib, stitch as ST
    crop, target, coef, _ = _paste_case(G, "inside")
    buf = torch.zeros((41, 48, 3), dtype=torch.uint8, device=DEV)
    buf[:40].copy_(_dev(target))
    with pytest.raises(_lib.S2VError, match="overlap"):
        ST.paste_images(coef[None], _dev(crop)[None], buf[None, :40], out=buf[None, 1:])
    sq = torch.zeros((40, 40, 3), dtype=torch.uint8, device=DEV)
    with pytest.raises(_lib.S2VError, match="overlap"):
        ST.paste_images(coef[None], sq[None, :32, :32], torch.zeros_like(sq)[None], out=sq[None])       # crop inside out
    frame = _dev(_frame("inside"))
    with pytest.raises(_lib.S2VError, match="overlap"):
        ST.transform_quad(frame, _table(G, "inside"), 32, out=frame[None, :32, :32])
    assert torch.equal(buf[:40].cpu(), torch.from_numpy(target))         # nothing ran


# ----------------------------------------------------------------------------- the host path on top
@pytest.mark.parametrize("name", list(SC.QUAD_CASES))
def test_crop_image_and_paste_image_with_our_coefficients(G, name):
    from s2v_amd import stitch as ST
    W, H, S, quad = SC.QUAD_CASES[name]
    crop = ST.crop_image(_dev(_frame(name)), S, quad)
    assert np.array_equal(crop.cpu().numpy(), G[f"quad.{name}.crop"])
    inv = ST.calc_alignment_coefficients(quad + 0.5, ST.square(S))
    target = SC.image(f"{name}.target", H, W)
    got = ST.paste_image(inv, crop, _dev(target)).cpu().numpy()
    ref = G[f"paste.{name}.out"]
    print(f"{name}: {int((got != ref).any(2).sum())} pixels differ with our coefficients")
    assert np.array_equal(got, ref)


def test_crop_faces_by_quads_list_and_shrink_raises(G):
    from s2v_amd import stitch as ST
    files = [(None, _dev(_frame(n))) for n in SC.SMALL]
    crops, given = ST.crop_faces_by_quads(32, files, [SC.QUAD_CASES[n][3] for n in SC.SMALL])
    assert len(given) == 4 and crops.shape == (4, 32, 32, 3)
    for i, n in enumerate(SC.SMALL):
        assert np.array_equal(crops[i].cpu().numpy(), G[f"quad.{n}.crop"]), n
    W, H, S, quad = SC.SHRINK_QUAD
    with pytest.raises(ValueError, match="shrink"):
        ST.crop_image(_dev(SC.image("shrink", H, W)), S, quad)


def test_crop_faces_with_smoothing(G):
    """crop_faces with both sigmas: its quads are scipy's to the host bound (1e-9 px; another order of summation
    than scipy's, so not to the bit); the crops of the golden quads are bit-exact."""
    from s2v_amd import stitch as ST
    h, w = SC.SMOOTH_HW
    frames = _dev(np.stack([SC.image(f"smooth{i}", h, w) for i in range(6)]))
    crops, given, quads = ST.crop_faces(SC.SMOOTH_SIZE, (SC.SMOOTH_LMS, frames), scale=1.0,
                                        center_sigma=SC.SMOOTH_SIGMAS[0], xy_sigma=SC.SMOOTH_SIGMAS[1], use_fa=True)
    dq = np.abs(np.stack(quads) - G["smooth.quads"]).max()
    print(f"smoothed quads max |d| {dq:.2e} px")
    assert dq <= 1e-9 and crops.shape == (6, 32, 32, 3) and len(given) == 6
    crops, _ = ST.crop_faces_by_quads(SC.SMOOTH_SIZE, (SC.SMOOTH_LMS, frames), list(G["smooth.quads"]))
    assert np.array_equal(crops.cpu().numpy(), G["smooth.crops"])


def _stitcher(lms=SC.STITCH_LMS, size=SC.STITCH_SIZE):
    from s2v_amd import face3d, stitch as ST
    return ST.Stitcher(face3d.KeypointExtractor(SC.CannedDetector(lms)), image_size=size)


def test_stitcher_bit_exact_and_reuses_points_across_calls(G):
    ref, base = SC.stitch_inputs()
    ref_d = _dev(ref).permute(0, 3, 1, 2).contiguous()
    base_d = _dev(base)
    st = _stitcher()
    got = st(ref_d, base_d)
    assert got.shape == (3, 3, 64, 64) and st.misses == 1
    assert np.array_equal(got.permute(0, 2, 3, 1).cpu().numpy(), G["stitcher.out"])
    # its intermediate results: the landmarks with the reuse rule, their quads and the crops
    from s2v_amd import stitch as ST
    lms = _stitcher().landmarks(_dev(ref))
    assert lms.dtype == np.float32 and np.array_equal(lms[1], lms[0])
    crops, _, quads = ST.crop_faces(SC.STITCH_SIZE, (lms, _dev(ref)), scale=1.0, use_fa=True)
    assert np.array_equal(np.stack(quads), G["stitcher.quads"])
    assert np.array_equal(crops.cpu().numpy(), G["stitcher.crops"])
    # the same clip in batches of one: the frame without a face sits at a batch border
    st = _stitcher()
    parts = [st(ref_d[i:i + 1], base_d[i:i + 1]) for i in range(3)]
    assert torch.equal(torch.cat(parts), got) and st.misses == 1
    # after reset() the frame without a face has no predecessor: its quad is 0 / 0 and it raises
    st = _stitcher()
    st(ref_d[:1], base_d[:1])
    st.reset()
    with np.errstate(invalid="ignore"), pytest.raises(ValueError, match="non-finite"):
        st(ref_d[1:2], base_d[1:2])


# ----------------------------------------------------------------------------- pipeline and runner
def test_pipeline_stitch_stage():
    from helpers import synth_sd
    from s2v_amd import models, ops, synth
    from s2v_amd import pipeline as P
    dnet = models.DNet()
    dnet.load_state_dict(synth_sd("dnet"), strict=True)
    enet = models.ENet()
    enet.load_state_dict(synth_sd("enet"), strict=True)
    dnet, enet = dnet.eval(), enet.eval()
    b = 2
    src, coeff = synth.dnet_inputs("stitch.pipeline", b, 256)
    src, coeff = _dev(src), _dev(coeff)
    mel = _dev(synth.hash_array("stitch.pipeline.mel", (b, 1, 80, 16), -4.0, 4.0))
    lms = (SC.face_landmarks(128.0, 130.0, 150.0, 4.0), SC.face_landmarks(120.0, 126.0, 140.0, -7.0))

    def run(**kw):
        pipe = P.LipSyncPipeline(dnet, enet, device=DEV, batch=b, graph=False, **kw)
        out = torch.empty((b, 3, 384, 384), dtype=torch.uint8, device=DEV)
        pipe.run_batch(mel, src, coeff, out)
        return out.clone()

    with_stage = run(stitch=_stitcher(lms, 256))

    st = _stitcher(lms, 256)

    def by_hand(ref_u8):
        base = torch.empty_like(ref_u8)
        ops.S2V.to_u8_(src.contiguous(), base, -1.0, 1.0, 127.5, 1.0)
        return st(ref_u8, base.permute(0, 2, 3, 1).contiguous())

    assert torch.equal(with_stage, run(ref_hook=by_hand))
    without = run(stitch=None)
    assert not torch.equal(with_stage, without)
    # without the stage: exactly the launches run_batch made before it existed
    with torch.no_grad():
        fake = dnet(src, coeff, lane=0)["fake_image"]
        ref_u8 = torch.empty((b, 3, 256, 256), dtype=torch.uint8, device=DEV)
        face6 = torch.empty((b, 6, 256, 256), device=DEV)
        gt = torch.empty((b, 3, 256, 256), device=DEV)
        ops.S2V.lipsync_inputs_(src.contiguous(), fake, ref_u8, face6, gt)
        pred, _ = enet(mel, face6, gt, lane=0)
        today = torch.empty((b, 3, 384, 384), dtype=torch.uint8, device=DEV)
        ops.S2V.to_u8_(pred, today, 0.0, 1.0, 255.0, 0.0)
    assert torch.equal(without, today)
    # the uint8 target of the stage is the original crop face6 carries: (u8 / 255) in its first three planes
    base = torch.empty((b, 3, 256, 256), dtype=torch.uint8, device=DEV)
    ops.S2V.to_u8_(src.contiguous(), base, -1.0, 1.0, 127.5, 1.0)
    assert torch.equal(base[:, :, :128], (face6[:, :3, :128] * 255.0).round().to(torch.uint8))


def test_runner_stitch(tmp_path):
    from s2v_amd import inference
    face = str(write_mp4_header(tmp_path / "v.mp4", 128, 96, 12, 12800, 6144))          # 25 fps
    wav = str(write_wav(tmp_path / "a.wav", rate=16000, channels=1, seconds=0.5))
    lm = SC.face_landmarks(128.0, 130.0, 150.0, 3.0)
    det = SC.CannedDetector([lm, lm, None, SC.face_landmarks(126.0, 128.0, 146.0, -2.0)])
    r = inference.run(face, wav, max_frames=4, batch=4, stitch=True, stitch_detector=det)
    m = r["meta"]
    assert m["frames"] == 4 and m["frame_hw"] == [96, 128]
    assert m["stitch"] is True and m["stitch_misses"] == 1 and m["stitch_landmarks"] == "given detector"
    assert r["preds"].shape == (4, 3, 384, 384)
    plain = inference.run(face, wav, max_frames=4, batch=4)
    assert "stitch" not in plain["meta"] and not torch.equal(plain["preds"], r["preds"])
