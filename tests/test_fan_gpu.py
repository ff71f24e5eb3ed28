"""FAN landmark detection on the device: the four kernels of csrc/fan.hip against fp64 / NumPy
restatements and tests/golden/fan_goldens*.npz (recorded from the reference's own FAN, utils.crop and
get_preds_fromhm by tests/golden/make_fan_golden.py), models.FAN in every conv arithmetic mode,
face_detection.FaceAlignment's landmark methods and the --landmarks wiring of inference.run.

Bars:
* s2v_bn_act_nhwc: |d| <= 2^-22 (|x s| + |t|) against fp64 (one product and one sum, each rounded at most once);
* s2v_fan_merge: a k-term sum gets k 2^-23 sum|terms|; the pooled mean is a four-term sum scaled by the exact
  0.25: 4 2^-23 0.25 sum|terms| (terms: the four pixels' a and b values); an activated output gets its sum's
  bound times |scale| plus the affine bound 2^-22 (|s scale| + |shift|);
* s2v_fan_peaks: EXACTLY the recorded preds / a NumPy restatement of get_preds_fromhm on crafted maps;
* s2v_fan_crop: BIT-EXACT in uint8 against the reference's crops;
* FAN.forward: per stack max|d| <= 1e-3 max(1, max|ref|) (the detectors' bound) on the stored channels;
* end to end: every landmark the fixture marks ``decided`` (one position within 2 eps of the maximum, every
  neighbour difference that matters above 2 eps, eps the forward bound) gives exactly the fixture's point;
  every other landmark's argmax lies in the recorded near-maximal set, which the forward bound implies.
"""
import itertools

import numpy as np
import pytest
import torch

import fan_cases as FC
import s2v_import  # noqa: F401
from helpers import write_mp4_header, write_wav

pytestmark = pytest.mark.gpu
DEV = "cuda"
U22, U23 = 2.0 ** -22, 2.0 ** -23


def _lib():
    from s2v_amd import _lib
    return _lib.load(), _lib.check, torch.cuda.current_stream().cuda_stream


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


# ----------------------------------------------------------------------------- kernels
def test_bn_act_on_a_channel_slice_matches_fp64():
    lib, check, stream = _lib()
    pixels, c, x_cs, x_off, y_cs, y_off = 1 * 5 * 7, 64, 256, 128, 96, 32
    x = FC.synth.hash_array("fan.bn.x", (pixels, x_cs), -3.0, 3.0)
    s = FC.synth.hash_array("fan.bn.s", (c,), -2.0, 2.0)
    t = FC.synth.hash_array("fan.bn.t", (c,), -1.0, 1.0)
    xd, sd, td = _dev(x), _dev(s), _dev(t)
    yd = torch.full((pixels, y_cs), -7.0, device=DEV)
    check(lib.s2v_bn_act_nhwc(xd.data_ptr(), pixels, c, x_cs, x_off, sd.data_ptr(), td.data_ptr(), yd.data_ptr(), y_cs,
                              y_off, stream), "s2v_bn_act_nhwc")
    got = yd.cpu().numpy().astype(np.float64)
    xs = x[:, x_off:x_off + c].astype(np.float64) * s.astype(np.float64)
    ref = np.maximum(xs + t.astype(np.float64), 0.0)
    bound = U22 * (np.abs(xs) + np.abs(t.astype(np.float64)))
    err = np.abs(got[:, y_off:y_off + c] - ref)
    print(f"bn_act: max |d| / bound {np.max(err / bound):.3f}")
    assert (err <= bound).all() and (ref > 0).any() and (ref == 0).any()
    assert (got[:, :y_off] == -7.0).all() and (got[:, y_off + c:] == -7.0).all()      # nothing outside the view


def _merge_case(tag, n, h, w, c, b_mode):
    """Every output combination of one (shape, b) case; b_mode: None, 'full' or 'half'."""
    lib, check, stream = _lib()
    quad = h % 2 == 0 and w % 2 == 0
    a_cs, b_cs = c + 8, c + 4
    a = FC.synth.hash_array(f"{tag}.a", (n, h, w, a_cs), -4.0, 4.0)
    bshape = (n, h // 2, w // 2, b_cs) if b_mode == "half" else (n, h, w, b_cs)
    b = FC.synth.hash_array(f"{tag}.b", bshape, -4.0, 4.0) if b_mode else None
    sA, tA, sB, tB = (FC.synth.hash_array(f"{tag}.{k}", (c,), -2.0, 2.0) for k in ("sA", "tA", "sB", "tB"))
    a64 = a[..., :c].astype(np.float64)
    b64 = np.zeros_like(a64)
    if b_mode == "half":
        b64 = np.repeat(np.repeat(b[..., :c].astype(np.float64), 2, 1), 2, 2)       # nearest x2
    elif b_mode:
        b64 = b[..., :c].astype(np.float64)
    k = 2 if b_mode else 1
    s_ref = a64 + b64
    s_terms = np.abs(a64) + np.abs(b64)
    s_bound = (k * U23 * s_terms) if b_mode else np.zeros_like(s_terms)             # s = a is exact
    refs = {"s": (s_ref, s_bound)}
    A = lambda v: v.astype(np.float64)  # noqa: E731
    refs["sa"] = (np.maximum(s_ref * A(sA) + A(tA), 0),
                  s_bound * np.abs(A(sA)) + U22 * (np.abs(s_ref * A(sA)) + np.abs(A(tA))))
    if quad:
        pool = lambda v: v.reshape(n, h // 2, 2, w // 2, 2, c).sum((2, 4))  # noqa: E731
        p_ref = 0.25 * pool(s_ref)
        p_bound = 4 * U23 * 0.25 * pool(s_terms)
        refs["p"] = (p_ref, p_bound)
        refs["pa"] = (np.maximum(p_ref * A(sB) + A(tB), 0),
                      p_bound * np.abs(A(sB)) + U22 * (np.abs(p_ref * A(sB)) + np.abs(A(tB))))
    ad, bd = _dev(a), (_dev(b) if b_mode else None)
    sAd, tAd, sBd, tBd = (_dev(v) for v in (sA, tA, sB, tB))
    pitches = {"s": c, "sa": c + 4, "p": c + 12, "pa": c + 16}
    names = [k for k in ("s", "sa", "p", "pa") if k in refs]
    worst, combos = 0.0, 0
    for r in range(1, len(names) + 1):
        for combo in itertools.combinations(names, r):
            outs = {k: torch.full(refs[k][0].shape[:3] + (pitches[k],), -7.0, device=DEV) for k in combo}
            ptr = lambda k: (outs[k].data_ptr(), pitches[k]) if k in outs else (None, 0)  # noqa: E731
            check(lib.s2v_fan_merge(ad.data_ptr(), a_cs, bd.data_ptr() if b_mode else None, b_cs, int(b_mode == "half"),
                                    n, h, w, c, *ptr("s"), *ptr("sa"), sAd.data_ptr(), tAd.data_ptr(), *ptr("p"),
                                    *ptr("pa"), sBd.data_ptr(), tBd.data_ptr(), stream), "s2v_fan_merge")
            for kname in combo:
                got = outs[kname].cpu().numpy().astype(np.float64)
                ref, bound = refs[kname]
                err = np.abs(got[..., :c] - ref)
                assert (err <= bound).all(), (tag, combo, kname, float(err.max()))
                assert (got[..., c:] == -7.0).all(), (tag, combo, kname)
                nz = bound > 0
                worst = max(worst, float((err[nz] / bound[nz]).max()) if nz.any() else 0.0)
            combos += 1
    print(f"fan_merge {tag} b={b_mode}: {combos} output combinations, max |d| / bound {worst:.3f}")
    return combos


@pytest.mark.parametrize("b_mode", [None, "full", "half"])
def test_merge_every_output_combination_2x4x6(b_mode):
    assert _merge_case("fan.merge.246", 2, 4, 6, 32, b_mode) == 15


def test_merge_upsamples_1x1_to_2x2():
    assert _merge_case("fan.merge.up", 1, 2, 2, 32, "half") == 15


@pytest.mark.parametrize("b_mode", [None, "full"])
def test_merge_odd_sizes_take_the_per_pixel_path(b_mode):
    """1x1 and 3x5 maps (the hourglass bottom of a 64x64 input): the sum and its activation only."""
    assert _merge_case("fan.merge.odd", 2, 3, 5, 16, b_mode) == 3
    assert _merge_case("fan.merge.one", 1, 1, 1, 256, b_mode) == 3


def _peaks_numpy(hm):
    """get_preds_fromhm (utils.py:144-161) on NHWC float32 maps [B,64,64,C] -> (preds [B,C,2], maxima)."""
    B, H, W, C = hm.shape
    preds, vals = np.zeros((B, C, 2), np.float32), np.zeros((B, C), np.float32)
    for b in range(B):
        for j in range(C):
            m = hm[b, :, :, j]
            idx = int(m.reshape(-1).argmax())                           # the first maximum
            pY, pX = divmod(idx, W)
            x, y = np.float32(pX + 1), np.float32(pY + 1)
            if 0 < pX < 63 and 0 < pY < 63:
                x += np.float32(0.25) * np.sign(m[pY, pX + 1] - m[pY, pX - 1])
                y += np.float32(0.25) * np.sign(m[pY + 1, pX] - m[pY - 1, pX])
            preds[b, j] = (x - np.float32(0.5), y - np.float32(0.5))
            vals[b, j] = m[pY, pX]
    return preds, vals


def _run_peaks(hm, c):
    lib, check, stream = _lib()
    B, H, W, cs = hm.shape
    hd = _dev(hm)
    preds = torch.full((B, c, 2), -7.0, device=DEV)
    vals = torch.full((B, c), -7.0, device=DEV)
    check(lib.s2v_fan_peaks(hd.data_ptr(), B, H, W, c, cs, preds.data_ptr(), vals.data_ptr(), stream), "s2v_fan_peaks")
    return preds.cpu().numpy(), vals.cpu().numpy()


def test_peaks_on_the_fixture_heatmaps_equal_the_recorded_preds(golden):
    g = golden("fan_goldens")
    hm = np.ascontiguousarray(g["full_last"].transpose(0, 2, 3, 1))      # [1,64,64,17]: every fourth landmark
    preds, vals = _run_peaks(hm, hm.shape[3])
    assert np.array_equal(preds[0], g["full_preds"][::FC.CHANNEL_STEP])
    assert np.array_equal(vals[0], g["full_peak"][::FC.CHANNEL_STEP])


@pytest.mark.parametrize("cs", [68, 72])
def test_peaks_on_crafted_maps(cs):
    hm = FC.synth.hash_array(f"fan.peaks.{cs}", (2, 64, 64, cs), -1.0, 1.0)
    top = np.float32(5.0)

    def put(b, ch, *pts):
        for y, x in pts:
            hm[b, y, x, ch] = top
    put(0, 0, (30, 5), (10, 20))                         # two equal maxima: the lowest flat index (10, 20)
    put(0, 1, (6, 4), (6, 5))                            # neighbours, scanned by different waves
    put(0, 2, (6, 4), (6, 20))                           # 16 apart: scanned by the same wave
    for ch, pt in enumerate(((0, 0), (0, 63), (63, 0), (63, 63), (0, 17), (63, 40), (22, 0), (31, 63)), 3):
        put(0, ch, pt)                                   # corners and borders: no step
    put(0, 11, (20, 20))
    hm[0, 20, 19, 11] = hm[0, 20, 21, 11] = np.float32(0.5)      # zero x difference: no x step, y steps
    put(0, 12, (40, 41))
    hm[0, 39, 41, 12] = hm[0, 41, 41, 12] = np.float32(-0.25)    # zero y difference
    put(0, 13, (1, 1))
    put(0, 14, (62, 62))                                 # the last interior position
    put(0, 67, (33, 34))                                 # the last channel (second 64-channel chunk)
    put(1, 66, (63, 63), (0, 0))
    hm[1, :, :, 5] = np.float32(0.125)                   # a constant map: the first position
    ref_p, ref_v = _peaks_numpy(hm[..., :68])
    assert ref_p[0, 0].tolist() == [20.75 if hm[0, 10, 21, 0] > hm[0, 10, 19, 0] else 20.25,
                                    10.75 if hm[0, 11, 20, 0] > hm[0, 9, 20, 0] else 10.25]
    assert ref_p[0, 3].tolist() == [0.5, 0.5] and ref_p[0, 6].tolist() == [63.5, 63.5]
    assert ref_p[0, 11, 0] == 20.5 and ref_p[0, 12, 1] == 40.5 and ref_p[1, 5].tolist() == [0.5, 0.5]
    preds, vals = _run_peaks(hm, 68)
    assert np.array_equal(preds, ref_p) and np.array_equal(vals, ref_v)


def test_crop_matches_the_reference_bit_exactly(golden):
    from s2v_amd import face_detection as fd
    g, gc = golden("fan_goldens"), golden("fan_goldens_crop")
    frames = _dev(FC.frames(FC.CROP))
    fa = fd.FaceAlignment(fd.LandmarksType._2D, device=DEV, detector=object())
    x4 = fa.crops(frames, g["crop_table"])
    got = x4.t.cpu().numpy()
    want = gc["crop_out"]
    assert got.shape == (6, 256, 256, 4) and (got[..., 3] == 0).all()
    u8 = np.rint(got[..., :3] * 255.0).astype(np.int64)
    diff = np.abs(u8 - want.astype(np.int64))
    print(f"fan_crop: {int((diff != 0).sum())} of {diff.size} uint8 values differ (max {int(diff.max())})")
    assert np.array_equal(u8, want.astype(np.int64))
    assert np.array_equal(got[..., :3], want.astype(np.float32) / np.float32(255.0))    # float32(v) / 255
    assert (want[1][:, :40] == 0).all() and (want[5][:60] == 0).all()      # the zero-filled parts are in the fixture


# ----------------------------------------------------------------------------- network
@pytest.fixture(scope="module")
def net():
    from s2v_amd import models
    m = models.FAN()
    m.load_state_dict(FC.state_dict(), strict=True)
    return m.eval()


def _check_stack(tag, got, ref, ref_max):
    bound = FC.forward_eps(ref_max)
    err = float(np.abs(got - ref).max())
    print(f"fan forward {tag}: max|d| {err:.3e} (bound {bound:.3e}, max|ref| {ref_max:.3e})")
    assert got.shape == ref.shape and err <= bound, (tag, err, bound)


def test_fan_forward_matches_reference(golden, net, prec):
    gf, g = golden("fan_goldens_forward"), golden("fan_goldens")
    step = FC.CHANNEL_STEP
    outs = [o.cpu().numpy() for o in net(_dev(FC.net_input(FC.FORWARD)))]
    assert len(outs) == 4 and all(o.shape == (2, 68, 32, 32) for o in outs)
    for i in range(3):
        _check_stack(f"forward {prec} stack {i}", outs[i][:, ::step], gf[f"forward_stack{i}"], float(gf[f"forward_max{i}"]))
    _check_stack(f"forward {prec} stack 3 (full)", outs[3], gf["forward_last"], float(gf["forward_max3"]))
    full = net(_dev(FC.net_input(FC.FULL)))[-1].cpu().numpy()
    _check_stack(f"full {prec} last stack", full[:, ::step], g["full_last"], float(g["full_max"]))


def test_fan_rejects_sizes_before_any_launch(net):
    with pytest.raises(ValueError, match="multiples of 64"):
        net(torch.zeros(1, 3, 96, 128, device=DEV))


def _fa(net, **kw):
    from s2v_amd import face_detection as fd
    return fd.FaceAlignment(fd.LandmarksType._2D, device=DEV, detector=_NoDetector(), fan=net, **kw)


class _NoDetector:
    reference_scale = 195

    def detect_from_batch(self, images, flip=False):
        raise AssertionError("the boxes are given")


def test_end_to_end_on_the_full_crop(golden, net):
    from s2v_amd import face_detection as fd
    from s2v_amd.ops import NHWC
    g = golden("fan_goldens")
    x4 = torch.zeros((1, 256, 256, 4))
    x4[..., :3] = torch.from_numpy(FC.net_input(FC.FULL)).permute(0, 2, 3, 1)
    hm = net.heatmaps(NHWC(x4.to(DEV)))[0][fd.HEATMAP_STACK]
    preds, vals = _fa(net).peaks(hm)
    pts = fd.preds_to_image(preds[0], torch.tensor(FC.FULL_CENTER), FC.FULL_SCALE, 64).numpy()
    decided, sets, count = g["full_decided"], g["full_sets"], g["full_count"]
    eps = FC.forward_eps(float(g["full_max"]))
    assert decided.sum() >= 34
    for j in range(68):
        px, py = preds[0, j].numpy()
        pos = int(round(float(py) - 0.5)) * 64 + int(round(float(px) - 0.5))    # the steps are +-0.25: rounding undoes them
        assert abs(float(vals[0, j]) - float(g["full_peak"][j])) <= eps, (j, float(vals[0, j]), g["full_peak"][j])
        if decided[j]:
            assert np.array_equal(preds[0, j].numpy(), g["full_preds"][j]), (j, preds[0, j], g["full_preds"][j])
            assert np.array_equal(pts[j], g["full_preds_orig"][j]), (j, pts[j], g["full_preds_orig"][j])
        else:
            assert pos in set(sets[j, : count[j]].tolist()), (j, pos, sets[j, : count[j]])
    print(f"fan end to end: {int(decided.sum())} decided landmarks exact, {int((~decided).sum())} inside their sets")


def _allowed_points(fd, sets, count, center, scale):
    """Frame points a landmark may map to: every near-maximal position with every quarter-pixel step."""
    out = []
    for j in range(68):
        cand = []
        for pos in sets[j, : count[j]].tolist():
            pY, pX = divmod(pos, 64)
            for sx, sy in itertools.product((-0.25, 0.0, 0.25), repeat=2):
                cand.append((pX + 1 + sx - 0.5, pY + 1 + sy - 0.5))
        pts = fd.preds_to_image(torch.tensor(cand, dtype=torch.float32), center, scale, 64).numpy()
        out.append({tuple(p) for p in pts.tolist()})
    return out


def test_get_landmarks_from_image_matches_the_glue_fixture(golden, net):
    from s2v_amd import face_detection as fd
    g = golden("fan_goldens")
    frame = FC.frames(FC.FULL)[0]
    fa = _fa(net)
    boxes = [np.asarray(b, np.float32) for b in FC.GLUE_BOXES]
    lms = fa.get_landmarks_from_image(frame, detected_faces=boxes)
    assert len(lms) == 2 and all(l.shape == (68, 2) and l.dtype == np.float32 for l in lms)
    for b, box in enumerate(boxes):
        decided = g[f"glue{b}_decided"]
        c, s = fd.box_center_scale(box)
        allowed = _allowed_points(fd, g[f"glue{b}_sets"], g[f"glue{b}_count"], c, s)
        for j in range(68):
            if decided[j]:
                assert np.array_equal(lms[b][j], g[f"glue{b}_pts"][j]), (b, j, lms[b][j], g[f"glue{b}_pts"][j])
            else:
                assert tuple(lms[b][j].tolist()) in allowed[j], (b, j, lms[b][j])
        print(f"glue box {b}: {int(decided.sum())} decided landmarks exact")
    # the batch form: one entry per image, None without a face, the detector's order kept
    batch = np.stack([frame, frame, frame])
    res = fa.get_landmarks_from_batch(batch, detected_faces=[[boxes[1]], [], [boxes[0], boxes[1]]])
    assert res[1] is None and len(res[0]) == 1 and len(res[2]) == 2
    assert np.array_equal(res[0][0], lms[1]) and np.array_equal(res[2][0], lms[0]) and np.array_equal(res[2][1], lms[1])
    assert fa.get_landmarks_from_image(frame, detected_faces=[]) is None


def test_flip_input_runs_two_passes_and_an_identity_flip_equals_one_pass(net):
    """flip_input adds net(flip(inp)) flipped back through the column and landmark-pair tables.  With both
    tables the identity the second pass repeats the first, out = 2 hm, and the landmarks equal the single
    pass's exactly (doubling changes neither the argmax nor a difference's sign); with the real tables the
    result is a different set of points."""
    frame = FC.frames(FC.FULL)[0]
    boxes = [np.asarray(FC.GLUE_BOXES[0], np.float32)]
    one = _fa(net)
    single = one.get_landmarks_from_image(frame, detected_faces=boxes)[0]
    assert one.fan_passes == 1
    two = _fa(net, flip_input=True)
    two.flip_pairs = tuple(range(68))
    two.flip_columns = lambda width: range(width)
    same = two.get_landmarks_from_image(frame, detected_faces=boxes)[0]
    assert two.fan_passes == 2 and np.array_equal(same, single)
    real = _fa(net, flip_input=True)
    flipped = real.get_landmarks_from_image(frame, detected_faces=boxes)[0]
    assert real.fan_passes == 2 and flipped.shape == (68, 2) and not np.array_equal(flipped, single)


# ----------------------------------------------------------------------------- inference.run wiring
@pytest.fixture(scope="module")
def clip(tmp_path_factory):
    d = tmp_path_factory.mktemp("fan_clip")
    # 160 x 144: the synthetic S3FD's top box is face-sized here (on 200 x 180 noise it is a ~500 px box whose
    # landmarks give an align_img fit past the resize kernel's downscale limit: inference._usable_landmarks)
    mp4 = write_mp4_header(d / "v.mp4", 160, 144, 12, 12800, 6144)
    wav = write_wav(d / "a.wav", rate=16000, channels=1, seconds=0.5)
    return str(mp4), str(wav)


def test_cli_landmarks_run_reports_finite_coefficients_and_differs(clip, tmp_path, capsys):
    import json
    from s2v_amd import inference
    base = inference.run(*clip, max_frames=4, batch=4)                 # the all -1 landmark run
    assert "landmarks" not in base["meta"] and "semantic" not in base
    out = tmp_path / "lm.npz"
    assert inference.main(["--face", clip[0], "--audio", clip[1], "--max_frames", "4", "--LNet_batch_size", "4",
                           "--landmarks", "--outfile", str(out)]) == 0
    meta = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    print(f"--landmarks: {meta['landmark_misses']} frames without a face, {meta['landmark_rejects']} rejected fits")
    assert meta["landmarks"] == "2DFAN4 synthetic" and meta["frames"] == 4
    assert meta["landmark_misses"] == 0 and meta["landmark_rejects"] == 0
    saved = np.load(out)
    assert saved["semantic"].shape == (4, 262) and np.isfinite(saved["semantic"]).all()
    assert not np.array_equal(saved["preds"], base["preds"].cpu().numpy())     # other coefficients drive DNet
