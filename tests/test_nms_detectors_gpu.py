"""nms="device" in the three detectors and in inference.run: the same lists as nms="host", exactly.

The two paths share the network and the decode kernel, so they see bit-identical candidates; with no two
candidates of equal score (asserted first) the device NMS and py_cpu_nms must keep the same rows in the same
order, and the arithmetic after the NMS is the same NumPy on the same values."""
import numpy as np
import pytest
import torch

import nms_cases as NC
import s2v_import  # noqa: F401
import s3fd_cases as SC
from helpers import FACE_IMG_HW, retina_head_outputs, write_mp4_header, write_wav

pytestmark = pytest.mark.gpu
DEV = "cuda"


# ----------------------------------------------------------------------------- S3FD
@pytest.fixture(scope="module")
def s3fd_net():
    from s2v_amd import models
    m = models.S3FD()
    m.load_state_dict(SC.state_dict(), strict=True)
    return m.eval()


def _same_lists(a, b):
    return len(a) == len(b) and all(len(x) == len(y) and all(np.array_equal(p, q) for p, q in zip(x, y))
                                    for x, y in zip(a, b))


def test_sfd_detector_device_nms_equals_host(s3fd_net):
    from s2v_amd import face_detection
    frames = SC.frames("small")                                            # 2 x 64 x 64: the smallest case
    host = face_detection.SFDDetector(DEV, net=s3fd_net)
    dev = face_detection.SFDDetector(DEV, net=s3fd_net, nms="device")
    assert host.nms == "host" and dev.nms == "device"
    for rows in host.candidates(host.head_maps(frames, flip=True)):
        assert len(rows) > 20 and len(np.unique(rows[:, 5])) == len(rows)  # no score ties among the candidates
    exp = host.detect_from_batch(frames, flip=True)
    got = dev.detect_from_batch(frames, flip=True)
    assert all(len(d) > 0 for d in exp) and _same_lists(got, exp)
    assert all(isinstance(d, list) and d[0].dtype == np.float32 and d[0].shape == (5,) for d in got)
    # the rect path on top of it, and a single image
    fa_h = face_detection.FaceAlignment(face_detection.LandmarksType._2D, device=DEV, detector=host)
    fa_d = face_detection.FaceAlignment(face_detection.LandmarksType._2D, device=DEV, detector=dev)
    assert fa_d.get_detections_for_batch(frames) == fa_h.get_detections_for_batch(frames)
    assert _same_lists([dev.detect_from_image(frames[0])], [host.detect_from_image(frames[0])])
    # an image with more kept boxes than keep_max takes the host path alone: the same lists again
    few = face_detection.SFDDetector(DEV, net=s3fd_net, nms="device", keep_max=1)
    assert max(len(d) for d in exp) > 1
    assert _same_lists(few.detect_from_batch(frames, flip=True), exp)


# ----------------------------------------------------------------------------- RetinaFace
def _retina_maps(hw=FACE_IMG_HW):
    """helpers.retina_head_outputs (clusters of confident, overlapping anchors) laid out as the fused NHWC head
    maps s2v_retina_decode reads: [box a0 | box a1 | cls a0 | cls a1 | lm a0 | lm a1] per pixel, 32 channels;
    the class logits are (log(1 - s), log(s)), whose softmax is (1 - s, s) up to rounding."""
    from s2v_amd.ops import NHWC
    loc, conf, lm = retina_head_outputs(hw)
    logit = np.log(np.maximum(conf.astype(np.float64), 1e-30)).astype(np.float32)
    maps, first = [], 0
    for s in (8, 16, 32):
        h, w = -(-hw[0] // s), -(-hw[1] // s)
        p = 2 * h * w
        m = np.zeros((1, h, w, 32), np.float32)
        m[0, ..., 0:8] = loc[first: first + p].reshape(h, w, 8)
        m[0, ..., 8:12] = logit[first: first + p].reshape(h, w, 4)
        m[0, ..., 12:32] = lm[first: first + p].reshape(h, w, 20)
        maps.append(NHWC(torch.from_numpy(m).to(DEV)))
        first += p
    assert first == len(loc)
    return maps


@pytest.fixture(scope="module")
def retina_maps():
    return _retina_maps()


def _retina(cls, maps, **kw):
    det = cls(device=DEV, net=torch.nn.Identity(), **kw)
    (det.det if hasattr(det, "det") else det).head_maps = lambda img: maps
    return det


def test_retinaface_detect_device_nms_equals_host(retina_maps):
    from s2v_amd import face
    img = np.zeros(FACE_IMG_HW + (3,), np.uint8)
    host = _retina(face.RetinaFaceDetection, retina_maps)
    dev = _retina(face.RetinaFaceDetection, retina_maps, nms="device")
    for thr in (0.5, 0.9):
        boxes, scores, _ = host.candidates(retina_maps, *FACE_IMG_HW, thr)
        assert len(scores) > 20 and len(np.unique(scores)) == len(scores)  # no score ties among the candidates
    for kw in (dict(), dict(nms_threshold=0.3), dict(top_k=15), dict(keep_top_k=3), dict(confidence_threshold=0.5)):
        ed, el = host.detect(img, **kw)
        gd, gl = dev.detect(img, **kw)
        assert ed.dtype == gd.dtype == np.float32 and el.dtype == gl.dtype
        if not kw:
            assert 0 < len(ed) < len(scores)                               # the NMS suppresses some anchors
        assert np.array_equal(gd, ed) and np.array_equal(gl, el), kw
    assert len(host.detect(img, keep_top_k=3)[0]) == 3
    # resize != 1 rescales the boxes before the NMS: that call stays on the host
    calls = []
    dev.kept_rows = lambda *a, **k: calls.append(a)
    ed, el = host.detect(img, resize=2)
    gd, gl = dev.detect(img, resize=2)
    assert not calls and np.array_equal(gd, ed) and np.array_equal(gl, el)


def test_retinaface_detect_faces_device_nms_equals_host(retina_maps):
    from s2v_amd import restore
    img = np.zeros(FACE_IMG_HW + (3,), np.uint8)
    host = _retina(restore.RetinaFaceDetector, retina_maps)
    dev = _retina(restore.RetinaFaceDetector, retina_maps, nms="device")
    for thr, iou in ((0.9, 0.4), (0.97, 0.4), (0.5, 0.3)):
        exp = host.detect_faces(img, thr, iou)
        got = dev.detect_faces(img, thr, iou)
        assert exp.shape[1] == 15 and len(exp) > 0 and got.dtype == exp.dtype
        assert np.array_equal(got, exp), (thr, iou)
    # more faces than keep_max: the host path serves the call
    few = _retina(restore.RetinaFaceDetector, retina_maps, nms="device", keep_max=2)
    exp = host.detect_faces(img, 0.9)
    assert len(exp) > 2 and np.array_equal(few.detect_faces(img, 0.9), exp)


def test_nms_device_reports_status_and_truncation(retina_maps):
    from s2v_amd import face
    det = _retina(face.RetinaFaceDetection, retina_maps)
    cand, count, p = det.decode(retina_maps, *FACE_IMG_HW, 0.9)
    (rows, status), = face.nms_device(cand, count, 1, p, 16, 0.4)
    slots = cand[: int(count.item()) * 16].view(-1, 16).cpu().numpy()
    exp = NC.by_py_cpu_nms(slots, 0.4)
    assert status == face.NMS_OK and np.array_equal(rows.view(np.uint32), exp.view(np.uint32))
    (rows, status), = face.nms_device(cand, count, 1, p, 16, 0.4, keep_max=2)
    assert status == face.NMS_TRUNCATED and np.array_equal(rows, exp[:2])
    cand2 = cand.clone()
    cand2[5] = float("nan")                                                # slot 0's score
    (rows, status), = face.nms_device(cand2, count, 1, p, 16, 0.4)
    assert status == face.NMS_NAN_SCORE and rows.shape == (0, 16)
    with pytest.raises(ValueError, match="nms_device"):
        face.nms_device(cand, count, 2, p, 16, 0.4)                        # the buffer holds one image


# ----------------------------------------------------------------------------- inference.run
def test_inference_face_det_device_nms_gives_the_same_boxes(tmp_path):
    from s2v_amd import inference
    mp4 = str(write_mp4_header(tmp_path / "v.mp4", 200, 180, 12, 12800, 6144))
    wav = str(write_wav(tmp_path / "a.wav", rate=16000, channels=1, seconds=0.5))
    det, _ = inference._face_detector(None, torch.device(DEV))
    frames = inference._frames(mp4, 2)[0]
    for rows in det.face_detector.candidates(det.face_detector.head_maps(frames, flip=True)):
        assert len(np.unique(rows[:, 5])) == len(rows)                     # no score ties among the candidates
    host = inference.run(mp4, wav, max_frames=2, batch=2, face_det=True, nosmooth=True, nms="host")
    dev = inference.run(mp4, wav, max_frames=2, batch=2, face_det=True, nosmooth=True, nms="device")
    assert host["meta"]["nms"] == "host" and dev["meta"]["nms"] == "device"
    assert dev["meta"]["boxes"] == host["meta"]["boxes"] and len(dev["meta"]["boxes"]) == 2
    assert torch.equal(dev["frames"], host["frames"]) and torch.equal(dev["preds"], host["preds"])
