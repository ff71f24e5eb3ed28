"""S3FD face detection, host side (s2v_amd.face_detection, models/s3fd_arch.py, the C ABI's argument
checks, the engine's host plan) against tests/golden/s3fd_goldens.npz, which
tests/golden/make_s3fd_golden.py recorded from the reference's own functions (net_s3fd.s3fd,
detect.batch_detect, bbox.nms, FaceAlignment.get_detections_for_batch, get_smoothened_boxes and
face_detect of futils/inference_utils.py)."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

import s2v_import  # noqa: F401
import s3fd_cases as SC

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


class _Stub:
    """get_detections_for_batch returning fixed rects in order; ``fail``: raise RuntimeError on the
    first ``fail`` calls (the reference's OOM recovery, which starts over from the first frame)."""

    def __init__(self, rects, fail=0):
        self.rects, self.fail, self.i, self.batches = list(rects), fail, 0, []

    def get_detections_for_batch(self, images):
        self.batches.append(len(images))
        if self.fail > 0:
            self.fail -= 1
            self.i = 0
            raise RuntimeError("out of memory")
        out = self.rects[self.i: self.i + len(images)]
        self.i += len(images)
        return out


def _fd_frames():
    return list(SC.synth.sr_frame("s3fd.fd", len(SC.FD_RECTS), *SC.FD_HW))


@pytest.mark.parametrize("name", sorted(SC.SMOOTH_CASES))
def test_get_smoothened_boxes_matches_reference(golden, name):
    from s2v_amd.face_detection import get_smoothened_boxes
    g = golden("s3fd_goldens")
    boxes = np.array(SC.SMOOTH_CASES[name])
    out = get_smoothened_boxes(boxes, 5)
    assert out is boxes and out.dtype == np.array([1]).dtype            # in place, on the integer array
    assert np.array_equal(out, g[name])
    assert not np.array_equal(g[name], np.array(SC.SMOOTH_CASES[name]))  # the case does smooth something


def test_get_smoothened_boxes_truncates_and_reads_smoothed_rows():
    from s2v_amd.face_detection import get_smoothened_boxes
    b = np.array([[0, 0, 0, 0], [1, 1, 1, 1], [4, 4, 4, 4]])
    # len 3 < T 5: every window is boxes[3 - 5:] = boxes[-2:], the last two rows, re-read after each
    # in-place assignment: row 0 = mean(1, 4) = 2.5 -> 2; row 1 = mean(1, 4) -> 2; row 2 = mean(2, 4) = 3
    # (the already smoothed row 1; the unsmoothed rows would give 2)
    out = get_smoothened_boxes(b, 5)
    assert out.tolist() == [[2, 2, 2, 2], [2, 2, 2, 2], [3, 3, 3, 3]]


@pytest.mark.parametrize("name,jaw,nosmooth", [("fd_default", False, False), ("fd_jaw", True, False),
                                               ("fd_jaw_nosmooth", True, True)])
def test_face_detect_boxes_match_reference(golden, name, jaw, nosmooth):
    from s2v_amd.face_detection import face_detect
    g = golden("s3fd_goldens")
    frames = _fd_frames()
    res = face_detect(frames, pads=SC.FD_PADS, nosmooth=nosmooth, jaw_correction=jaw, batch_size=4,
                      detector=_Stub(SC.FD_RECTS))
    coords = np.array([c for _, c in res])
    assert np.array_equal(coords, g[name])                               # (y1, y2, x1, x2) per frame
    for (crop, (y1, y2, x1, x2)), f in zip(res, frames):
        assert np.array_equal(crop, f[y1:y2, x1:x2])
    if name == "fd_jaw_nosmooth":
        # pads and clamping by hand: rect (36, 25, 119, 85) + pads (7, 12, 35, 9) in a 90x120 frame
        assert tuple(coords[3]) == (18, 90, 1, 120) and tuple(coords[2]) == (0, 87, 0, 79)
    if name == "fd_default":
        # jaw_correction=False ignores ``pads``: (0, 20, 0, 0)
        plain = face_detect(frames, pads=(0, 20, 0, 0), jaw_correction=True, detector=_Stub(SC.FD_RECTS))
        assert np.array_equal(np.array([c for _, c in plain]), coords)


def test_face_detect_takes_a_frame_array():
    from s2v_amd.face_detection import face_detect
    frames = _fd_frames()
    a = face_detect(frames, nosmooth=True, detector=_Stub(SC.FD_RECTS))
    b = face_detect(torch.from_numpy(np.stack(frames)), nosmooth=True, detector=_Stub(SC.FD_RECTS))
    assert [tuple(int(v) for v in c) for _, c in a] == [tuple(int(v) for v in c) for _, c in b]
    assert all(np.array_equal(x[0], y[0].numpy()) for x, y in zip(a, b))


def test_face_detect_no_face_raises_value_error(tmp_path, monkeypatch):
    from s2v_amd.face_detection import face_detect
    monkeypatch.chdir(tmp_path)
    rects = list(SC.FD_RECTS)
    rects[4] = None
    with pytest.raises(ValueError, match="Face not detected! Ensure the video contains a face in all the frames."):
        face_detect(_fd_frames(), detector=_Stub(rects))
    assert os.listdir(tmp_path) == []                                    # no faulty_frame file is written


def test_face_detect_halves_the_batch_on_runtime_error():
    from s2v_amd.face_detection import face_detect
    frames = _fd_frames()
    det = _Stub(SC.FD_RECTS, fail=1)
    res = face_detect(frames, nosmooth=True, batch_size=4, detector=det)
    assert det.batches == [4, 2, 2, 2]                                   # first batch fails; restart at 2
    ok = face_detect(frames, nosmooth=True, batch_size=4, detector=_Stub(SC.FD_RECTS))
    assert [c for _, c in res] == [c for _, c in ok]
    det = _Stub(SC.FD_RECTS, fail=10)
    with pytest.raises(RuntimeError, match="Image too big to run face detection on GPU. Please use the "
                                           "--resize_factor argument"):
        face_detect(frames, batch_size=4, detector=det)
    assert det.batches == [4, 2, 1]


@pytest.mark.parametrize("case", sorted(SC.CASES))
def test_nms_and_keep_on_own_candidates_match_reference(golden, case):
    """The per-image equivalence (face_detection's docstring): NMS(0.3) + score > 0.5 over an image's own
    candidates equals the reference's detect_from_batch over batch_detect's union rows."""
    from s2v_amd import face, face_detection
    g = golden("s3fd_goldens")
    for i in range(SC.CASES[case][1]):
        rows = g[f"{case}_cand{i}"]
        assert face.py_cpu_nms(rows, 0.3) == g[f"{case}_nms_keep{i}"].tolist()
        kept = np.array(face_detection.nms_keep(rows), np.float32).reshape(-1, 5)
        assert len(kept) and np.array_equal(kept, g[f"{case}_dets{i}"])
    assert face_detection.nms_keep(np.zeros((0, 5), np.float32)) == []


def test_get_detections_for_batch_clips_and_truncates(golden):
    from s2v_amd.face_detection import FaceAlignment, LandmarksType
    g = golden("s3fd_goldens")
    seen = {}

    class _Sfd:
        def detect_from_batch(self, images, flip=False):
            seen["flip"], seen["shape"] = flip, tuple(images.shape)
            return [list(g[f"main_dets{i}"]) for i in range(3)] + [[]]

    fa = FaceAlignment(LandmarksType._2D, device="cpu", flip_input=False, detector=_Sfd())
    rects = fa.get_detections_for_batch(np.zeros((4, 137, 181, 3), np.uint8))
    assert seen == {"flip": True, "shape": (4, 137, 181, 3)}
    assert rects[3] is None
    for i in range(3):
        assert rects[i] == tuple(g[f"main_rect{i}"].tolist()) and all(isinstance(v, int) for v in rects[i])
    assert any(g[f"main_dets{i}"][0, :4].min() < 0 and min(rects[i]) == 0 for i in range(3))   # a clipped box
    assert LandmarksType._2D.value == 1 and LandmarksType._3D.value == 3


def test_sfd_detector_needs_weights_and_keeps_reference_properties():
    from s2v_amd import face_detection, models
    with pytest.raises(FileNotFoundError):
        face_detection.SFDDetector("cpu")                                # never downloads
    det = face_detection.SFDDetector("cpu", net=models.S3FD())
    assert (det.reference_scale, det.reference_x_shift, det.reference_y_shift) == (195, 0, 0)


def test_state_dict_manifest_is_strict():
    from s2v_amd import models
    from s2v_amd.models.s3fd_arch import S3FDParams
    with open(os.path.join(GOLDEN, "s3fd_keys.json")) as f:
        want = json.load(f)
    assert len(want) == 65
    mine = {k: list(v.shape) for k, v in S3FDParams().state_dict().items()}
    assert mine == want
    net = models.S3FD()
    sd = dict(SC.state_dict())
    net.load_state_dict(sd, strict=True)
    del sd["conv4_3_norm.weight"]
    with pytest.raises(RuntimeError, match="conv4_3_norm.weight"):
        models.S3FD().load_state_dict(sd, strict=True)
    sd = dict(SC.state_dict(), extra=torch.zeros(1))
    with pytest.raises(RuntimeError, match="extra"):
        models.S3FD().load_state_dict(sd, strict=True)


def test_load_s3fd_is_strict(tmp_path):
    from s2v_amd import models
    torch.save(SC.state_dict(), tmp_path / "s3fd.pth")
    net = models.load_s3fd(str(tmp_path / "s3fd.pth"))
    assert not net.training and torch.equal(net.fc7.bias, SC.state_dict()["fc7.bias"])
    sd = {k: v for k, v in SC.state_dict().items() if k != "fc6.bias"}
    torch.save(sd, tmp_path / "bad.pth")
    with pytest.raises(RuntimeError, match="fc6.bias"):
        models.load_s3fd(str(tmp_path / "bad.pth"))


def test_level_sizes_and_too_small_inputs():
    from s2v_amd.models import s3fd_arch
    assert s3fd_arch.level_sizes(137, 181) == [(34, 45), (17, 22), (8, 11), (8, 9), (4, 5), (2, 3)]
    assert s3fd_arch.level_sizes(64, 64) == [(16, 16), (8, 8), (4, 4), (6, 6), (3, 3), (2, 2)]
    assert s3fd_arch.level_sizes(32, 32)[-1] == (2, 2)
    for hw in ((31, 64), (64, 31), (8, 8)):
        with pytest.raises(ValueError, match="too small"):
            s3fd_arch.level_sizes(*hw)


def test_fixture_map_shapes_follow_level_sizes(golden):
    from s2v_amd.models import s3fd_arch
    g = golden("s3fd_goldens")
    for case, (_, n, h, w) in SC.CASES.items():
        for lv, (lh, lw) in enumerate(s3fd_arch.level_sizes(h, w)):
            assert g[f"{case}_map{2 * lv}"].shape == (n, 2, lh, lw) and g[f"{case}_map{2 * lv + 1}"].shape == (n, 4, lh, lw)


def test_s3fd_entry_points_reject_bad_arguments():
    from s2v_amd import _lib
    lib = _lib.load()
    p = lambda a: a.ctypes.data  # noqa: E731
    x = np.zeros(64 * 16, np.float32)
    y = np.zeros(64 * 16, np.float32)
    w = np.zeros(64, np.float32)
    u8 = np.zeros(4 * 4 * 3, np.uint8)
    assert x.ctypes.data % 16 == 0 and y.ctypes.data % 16 == 0 and w.ctypes.data % 16 == 0
    # l2norm: null pointers, c % 4, pitch below c / not a multiple of 4, too many channels
    assert lib.s2v_l2norm_nhwc(None, 4, 16, 16, p(w), 1e-10, p(y), 16, None) == -1
    assert lib.s2v_l2norm_nhwc(p(x), 4, 16, 16, None, 1e-10, p(y), 16, None) == -1
    assert lib.s2v_l2norm_nhwc(p(x), 4, 16, 16, p(w), 1e-10, None, 16, None) == -1
    assert lib.s2v_l2norm_nhwc(p(x), 4, 18, 20, p(w), 1e-10, p(y), 20, None) == -1
    assert b"multiple of 4" in lib.s2v_last_error()
    assert lib.s2v_l2norm_nhwc(p(x), 4, 16, 12, p(w), 1e-10, p(y), 16, None) == -1
    assert lib.s2v_l2norm_nhwc(p(x), 4, 16, 16, p(w), 1e-10, p(y), 18, None) == -1
    assert lib.s2v_l2norm_nhwc(p(x), 0, 16, 16, p(w), 1e-10, p(y), 16, None) == -1
    assert lib.s2v_l2norm_nhwc(p(x), 1, 1028, 1028, p(w), 1e-10, p(y), 1028, None) == -1
    # u8_mean_nhwc4: null pointers, bad flip, empty batch
    mean = (ctypes.c_float * 3)(104, 117, 123)
    assert lib.s2v_u8_mean_nhwc4(None, 1, 16, mean, 0, p(y), None) == -1
    assert lib.s2v_u8_mean_nhwc4(p(u8), 1, 16, None, 0, p(y), None) == -1
    assert lib.s2v_u8_mean_nhwc4(p(u8), 1, 16, mean, 0, None, None) == -1
    assert lib.s2v_u8_mean_nhwc4(p(u8), 1, 16, mean, 2, p(y), None) == -1
    assert lib.s2v_u8_mean_nhwc4(p(u8), 0, 16, mean, 0, p(y), None) == -1
    # s3fd_decode: null pointers, a level with h <= 0, max_cand below the positions, cs below 8
    heads = (ctypes.c_void_p * 6)(*[p(x)] * 6)
    hs = (ctypes.c_int * 6)(5, 3, 2, 6, 3, 1)
    ws = (ctypes.c_int * 6)(7, 4, 2, 6, 3, 1)
    P = sum(a * b for a, b in zip(hs, ws))
    cand = np.zeros(2 * P * 8, np.float32)
    cnt = np.zeros(2, np.int32)
    assert lib.s2v_s3fd_decode(None, hs, ws, 8, 2, 0.05, p(cand), p(cnt), P, None) == -1
    assert lib.s2v_s3fd_decode(heads, hs, ws, 8, 2, 0.05, None, p(cnt), P, None) == -1
    assert lib.s2v_s3fd_decode(heads, hs, ws, 8, 2, 0.05, p(cand), None, P, None) == -1
    assert lib.s2v_s3fd_decode(heads, hs, ws, 8, 2, 0.05, p(cand), p(cnt), P - 1, None) == -1
    assert b"max_cand" in lib.s2v_last_error()
    assert lib.s2v_s3fd_decode(heads, hs, ws, 4, 2, 0.05, p(cand), p(cnt), P, None) == -1
    assert lib.s2v_s3fd_decode(heads, hs, ws, 8, 0, 0.05, p(cand), p(cnt), P, None) == -1
    bad_h = (ctypes.c_int * 6)(5, 3, 0, 6, 3, 1)
    assert lib.s2v_s3fd_decode(heads, bad_h, ws, 8, 2, 0.05, p(cand), p(cnt), P, None) == -1
    assert b"level 2" in lib.s2v_last_error()
    missing = (ctypes.c_void_p * 6)(p(x), p(x), p(x), None, p(x), p(x))
    assert lib.s2v_s3fd_decode(missing, hs, ws, 8, 2, 0.05, p(cand), p(cnt), P, None) == -1
    assert b"level 3" in lib.s2v_last_error()


def test_cli_parser_accepts_the_face_det_flags():
    from s2v_amd import inference
    ap = inference.build_parser()
    a = ap.parse_args(["--face", "v.mp4", "--audio", "a.wav"])
    assert (a.face_det, a.pads, a.nosmooth, a.face_det_batch_size) == (False, [0, 20, 0, 0], False, 4)
    a = ap.parse_args(["--face", "v.mp4", "--audio", "a.wav", "--face_det", "--pads", "5", "30", "2", "3", "--nosmooth",
                       "--face_det_batch_size", "2"])
    assert (a.face_det, a.pads, a.nosmooth, a.face_det_batch_size) == (True, [5, 30, 2, 3], True, 2)
    import inspect
    sig = inspect.signature(inference.run).parameters
    assert sig["face_det"].default is False and sig["detector"].default is None
    assert tuple(sig["pads"].default) == (0, 20, 0, 0) and sig["face_det_batch_size"].default == 4


# ----------------------------------------------------------------------------- engine host plan
def test_s3fd_engine_plan_runs_dry(monkeypatch):
    """The engine's shape / view bookkeeping on CPU with no-op launches (as test_engine_dryrun.py): 19
    trunk convs + 6 fused head convs, 5 pools, 3 L2 norms; a too small input raises before any launch."""
    from test_engine_dryrun import _NoLib, _NoOps
    from s2v_amd import ops
    from s2v_amd.engine.s3fd import S3FDEngine
    lib = _NoLib()
    monkeypatch.setattr(ops, "S2V", _NoOps(lib.calls))
    monkeypatch.setattr(ops, "_require_cuda", lambda t, what: None)
    monkeypatch.setattr(ops._lib, "load", lambda: lib)
    monkeypatch.setattr(ops.Ctx, "stream", property(lambda self: ctypes.c_void_p(0)))
    eng = S3FDEngine(SC.state_dict(), "cpu")
    ctx = ops.Ctx("cpu")
    maps = eng.forward_maps(ctx, ops.NHWC(torch.zeros(3, 137, 181, 4)))
    assert [(m.h, m.w, m.cs) for m in maps] == [(34, 45, 8), (17, 22, 8), (8, 11, 8), (8, 9, 8), (4, 5, 8), (2, 3, 8)]
    assert lib.calls["conv2d_"] == 25 and lib.calls["s2v_maxpool2d_nhwc"] == 5 and lib.calls["s2v_l2norm_nhwc"] == 3
    outs = eng.split_heads(maps)
    assert [tuple(o.shape) for o in outs[:4]] == [(3, 2, 34, 45), (3, 4, 34, 45), (3, 2, 17, 22), (3, 4, 17, 22)]
    before = dict(lib.calls)
    with pytest.raises(ValueError, match="too small"):
        eng.forward_maps(ctx, ops.NHWC(torch.zeros(1, 31, 40, 4)))
    assert lib.calls == before
