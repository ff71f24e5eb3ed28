"""The geometry between the preprocessing networks on the device (csrc/geom.hip): s2v_fan_landmarks,
s2v_face3d_align and s2v_dnet_windows against the case module tests/geom_cases.py (whose NumPy restatements
test_geom_cases_host.py pins to the host routes), the Python routes over them against the host routes, and
inference.run with geometry="device" against "host".

Bars:
* s2v_fan_landmarks: EXACTLY face_detection.preds_to_image;
* s2v_face3d_align: boxes and status EXACTLY the host route's (frame_landmarks + align_params with
  inference._usable_landmarks' verdict), trans within 1 float32 step: both routes are float64 and agree to
  ~1e-12 relative, so their float32 roundings differ by one step at most; the same s2v_pil_resize_crop image;
* s2v_dnet_windows: EXACTLY pipeline.dnet_coefficients;
* Face3DExtractor.semantic_device: trans_params within 1 step; the coefficient columns equal the host route's
  where the boxes are equal (the same launches on the same inputs);
* the CLI: the same reject count, semantic as above, frames within 1 grey level.
"""
import json

import numpy as np
import pytest
import torch

import fan_cases as FC
import geom_cases as GC
import s2v_import  # noqa: F401
from helpers import face3d_frames, synth_sd, write_mp4_header, write_wav

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _lib():
    from s2v_amd import _lib
    return _lib.load(), _lib.check, torch.cuda.current_stream().cuda_stream


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


class _NoDetector:
    reference_scale = 195

    def detect_from_batch(self, images, flip=False):
        raise AssertionError("the boxes are given")


def _fa(net=None, **kw):
    from s2v_amd import face_detection as fd
    return fd.FaceAlignment(fd.LandmarksType._2D, device=DEV, detector=_NoDetector(), fan=net, **kw)


# ----------------------------------------------------------------------------- landmarks
def test_fan_landmarks_equal_preds_to_image_exactly():
    lib, check, stream = _lib()
    faces = GC.landmark_faces()[1:]                        # 3 faces: halves, the corner window, m[2][2] != 1
    preds = GC.landmark_preds(4)[1:]
    mats = GC.landmark_mats(faces)
    pd, md = _dev(preds), _dev(mats)
    out = torch.full((3, 68, 2), -7.0, device=DEV)
    check(lib.s2v_fan_landmarks(pd.data_ptr(), md.data_ptr(), 3, 68, out.data_ptr(), stream), "s2v_fan_landmarks")
    got = out.cpu().numpy()
    assert np.array_equal(got, GC.landmarks_numpy(preds, mats))
    assert np.array_equal(got, GC.landmarks_host(preds, faces))
    assert (got < 0).any()


def test_fan_landmarks_on_integer_results_and_through_peaks_with_a_padded_stride():
    """k = 5 landmarks in heatmaps of channel pitch 8, peaks left on the device, the integer-centre face first:
    its results are exact integers, where a fused or a float64 sum would round differently."""
    from s2v_amd.ops import NHWC
    faces = GC.landmark_faces()[:3]
    hm = FC.synth.hash_array("geom.peaks", (3, 64, 64, 8), -1.0, 1.0)
    want_preds = GC.landmark_preds(3, k=5, key="geom.lm.k5")
    for f in range(3):
        for j in range(5):
            x, y = want_preds[f, j]
            pX, pY = int(np.floor(x - 0.5 + 0.25)), int(np.floor(y - 0.5 + 0.25))      # undo the quarter step
            hm[f, pY, pX, j] = 5.0
            if 0 < pX < 63 and 0 < pY < 63:
                sx, sy = x - (pX + 0.5), y - (pY + 0.5)
                hm[f, pY, pX + 1, j], hm[f, pY, pX - 1, j] = 1.0 + sx, 1.0 - sx
                hm[f, pY + 1, pX, j], hm[f, pY - 1, pX, j] = 1.0 + sy, 1.0 - sy
    fa = _fa()
    hd = NHWC(_dev(hm))
    preds, vals = fa.peaks(hd, on_device=True, k=5)
    assert preds.is_cuda and vals.is_cuda and preds.shape == (3, 5, 2) and vals.shape == (3, 5)
    host_preds, host_vals = fa.peaks(hd, k=5)
    assert np.array_equal(preds.cpu().numpy(), want_preds) and np.array_equal(host_preds.numpy(), want_preds)
    assert np.array_equal(vals.cpu().numpy(), host_vals.numpy())
    got = fa.landmarks_device(preds, _dev(GC.landmark_mats(faces))).cpu().numpy()
    assert np.array_equal(got, GC.landmarks_host(want_preds, faces))
    cx, cy, _ = faces[0]
    assert np.array_equal(got[0], 4.0 * want_preds[0] + np.array([cx - 128.0, cy - 128.0], np.float32))


def test_fan_landmarks_rejects_bad_arguments():
    lib, _, stream = _lib()
    t = torch.zeros(12, device=DEV)
    assert lib.s2v_fan_landmarks(None, t.data_ptr(), 1, 1, t.data_ptr(), stream) != 0
    assert lib.s2v_fan_landmarks(t.data_ptr(), t.data_ptr(), 0, 68, t.data_ptr(), stream) != 0


# ----------------------------------------------------------------------------- align
def _align_frames(size):
    W, H = size
    if (H, W) == (180, 240):
        return face3d_frames(6)
    return np.random.default_rng(5).integers(0, 256, (6, H, W, 3), dtype=np.uint8)


@pytest.mark.parametrize("size", GC.ALIGN_SIZES)
def test_face3d_align_equals_the_host_route(size):
    from s2v_amd import face3d, ops
    from s2v_amd.ops import NHWC
    W, H = size
    lms = GC.align_landmarks(size)
    ctx = ops.Ctx(DEV)
    params, trans, status = face3d.align_device(ctx, _dev(lms), W, H, GC.LM3D)
    h_params, h_trans, h_status, _ = GC.align_host(lms, W, H)
    r_params, r_trans, r_status = GC.align_numpy(lms, W, H)
    got_p, got_t, got_s = params.cpu().numpy(), trans.cpu().numpy(), status.cpu().numpy()
    assert got_s.tolist() == list(GC.ALIGN_STATUS) and np.array_equal(got_s, h_status)
    assert np.array_equal(got_p, h_params) and np.array_equal(got_p, r_params)
    u = GC.ulps(got_t, h_trans)
    print(f"face3d_align {W}x{H}: trans within {int(u.max())} float32 steps of the host route, "
          f"{int(GC.ulps(got_t, r_trans).max())} of the restatement")
    assert u.max() <= 1
    assert np.array_equal(got_t[3:], h_trans[3:])          # the frames on the no-landmark fit: the host's own values
    # the same network input from the device-made parameters as from the host-made ones
    frames = _dev(_align_frames(size))
    a, b = NHWC.empty(6, 224, 224, 4, DEV), NHWC.empty(6, 224, 224, 4, DEV)
    face3d.resize_crop_params(ctx, frames, params, a)
    face3d.resize_crop(ctx, frames, [tuple(int(v) for v in p) for p in h_params], b)
    assert torch.equal(a.t, b.t) and bool(torch.isfinite(a.t).all()) and float(a.t[:3].abs().max()) > 0


def test_face3d_align_rejects_bad_arguments():
    from s2v_amd import face3d, ops
    ctx = ops.Ctx(DEV)
    with pytest.raises(RuntimeError):
        face3d.align_device(ctx, torch.zeros((2, 68, 2)), 240, 180, GC.LM3D)
    with pytest.raises(RuntimeError):
        face3d.align_device(ctx, torch.zeros((2, 5, 2), device=DEV), 240, 180, GC.LM3D)
    p, t, s = face3d.align_device(ctx, torch.zeros((0, 68, 2), device=DEV), 240, 180, GC.LM3D)
    assert p.shape == (0, 4) and t.shape == (0, 5) and s.shape == (0,)


# ----------------------------------------------------------------------------- windows
@pytest.mark.parametrize("N", GC.WINDOW_CLIPS)
def test_dnet_windows_equal_dnet_coefficients_exactly(N):
    from s2v_amd import pipeline
    sem = GC.window_semantic(N)
    sd = _dev(sem)
    runs = 0
    for start, stop in GC.window_ranges(N):
        for exp in (None, GC.window_expression()):
            for one_shot in (False, True):
                got = pipeline.dnet_coefficients_device(sd, exp, one_shot, start, stop)
                assert got.is_cuda and got.shape == (stop - start, 73, 26)
                with np.errstate(all="ignore"):
                    want = pipeline.dnet_coefficients(sem, exp, one_shot, start, stop)
                assert np.array_equal(got.cpu().numpy(), want, equal_nan=True), (N, start, stop, exp is None, one_shot)
                assert np.array_equal(want, GC.windows_numpy(sem, exp, one_shot, start, stop), equal_nan=True)
                runs += 1
    assert runs == 4 * len(GC.window_ranges(N))
    assert pipeline.dnet_coefficients_device(sd, None, False, 2, 2).shape == (0, 73, 26)
    with pytest.raises(ValueError):
        pipeline.dnet_coefficients_device(sd, None, False, 0, N + 1)
    with pytest.raises(RuntimeError):
        pipeline.dnet_coefficients_device(torch.from_numpy(sem), None, False, 0, N)


# ----------------------------------------------------------------------------- routes
@pytest.fixture(scope="module")
def recon():
    from s2v_amd import models
    m = models.define_net_recon("resnet50", use_last_fc=False, init_path="")
    m.load_state_dict(synth_sd("recon"), strict=True)
    return m.eval()


def test_semantic_device_equals_face_3dmm_extraction(recon):
    from s2v_amd import face3d, inference
    W, H = GC.ALIGN_SIZES[0]
    lms = GC.align_landmarks((W, H))
    frames = _dev(face3d_frames(6))
    ext = face3d.Face3DExtractor(recon, GC.LM3D, DEV, batch=4)            # ragged last batch (4 + 2)
    sem, status = ext.semantic_device(frames, _dev(lms))
    assert sem.is_cuda and sem.shape == (6, 262) and status.cpu().tolist() == list(GC.ALIGN_STATUS)
    usable, rejects = inference._usable_landmarks(lms, H, W, GC.LM3D)     # the host route, as inference.run takes it
    want = ext.face_3dmm_extraction(frames, usable)
    got = sem.cpu().numpy()
    assert rejects == int((status == face3d.ALIGN_REJECTED).sum())
    assert GC.ulps(got[:, 257:], want[:, 257:]).max() <= 1
    d = np.abs(got[:, :257] - want[:, :257]).max()
    print(f"semantic_device: coefficient columns differ from the host route's by at most {d:.3e}")
    assert np.array_equal(got[:, :257], want[:, :257])                   # equal boxes: the same launches and inputs


@pytest.fixture(scope="module")
def net():
    from s2v_amd import models
    m = models.FAN()
    m.load_state_dict(FC.state_dict(), strict=True)
    return m.eval()


@pytest.mark.parametrize("flip_input", [False, True])
def test_get_landmarks_on_device_equals_the_host_call(net, flip_input):
    frame = FC.frames(FC.FULL)[0]
    boxes = [np.asarray(b, np.float32) for b in FC.GLUE_BOXES]
    batch = np.stack([frame, frame, frame])
    faces = [[boxes[1]], [], [boxes[0], boxes[1]]]
    fa = _fa(net, flip_input=flip_input)
    want = fa.get_landmarks_from_batch(batch, detected_faces=faces)
    passes = fa.fan_passes
    pts, index = fa.get_landmarks_from_batch(batch, detected_faces=faces, on_device=True)
    assert fa.fan_passes == 2 * passes and passes == (2 if flip_input else 1)
    assert pts.is_cuda and pts.shape == (3, 68, 2) and index == [0, 2, 2]
    got = pts.cpu().numpy()
    assert np.array_equal(got[0], want[0][0]) and np.array_equal(got[1], want[2][0]) and np.array_equal(got[2], want[2][1])
    none, index = fa.get_landmarks_from_batch(batch[:1], detected_faces=[[]], on_device=True)
    assert none.shape == (0, 68, 2) and index == []


def test_extract_keypoint_device_keeps_the_reference_rules(net):
    """Frames without a face: all -1 before the first face, the previous frame's points after it."""
    from s2v_amd import face3d
    frame = FC.frames(FC.FULL)[0]
    boxes = [np.asarray(b, np.float32) for b in FC.GLUE_BOXES]
    per_frame = [[], [boxes[0], boxes[1]], [], [boxes[1]], []]

    class Given:
        reference_scale = 195

        def __init__(self):
            self.k = 0

        def detect_from_batch(self, images, flip=False):
            out = per_frame[self.k: self.k + len(images)]
            self.k += len(images)
            return out
    frames = np.stack([frame] * len(per_frame))
    fa = _fa(net)
    fa.face_detector = Given()
    host = face3d.KeypointExtractor(fa, batch=2)
    want = host.extract_keypoint(frames, info=False)
    fa.face_detector = Given()
    dev = face3d.KeypointExtractor(fa, batch=2)
    got = dev.extract_keypoint_device(frames)
    assert got.is_cuda and got.dtype == torch.float32 and got.shape == (5, 68, 2)
    assert np.array_equal(got.cpu().numpy(), want.astype(np.float32)) and dev.misses == host.misses == 3
    assert (want[0] == -1).all() and np.array_equal(want[2], want[1]) and np.array_equal(want[4], want[3])


# ----------------------------------------------------------------------------- inference.run
@pytest.fixture(scope="module")
def clip(tmp_path_factory):
    d = tmp_path_factory.mktemp("geom_clip")
    mp4 = write_mp4_header(d / "v.mp4", 160, 144, 12, 12800, 6144)       # test_fan_gpu.py's plumbing clip, 8 frames
    wav = write_wav(d / "a.wav", rate=16000, channels=1, seconds=1.0)
    return str(mp4), str(wav)


def test_cli_geometry_device_equals_host(clip, tmp_path, capsys):
    from s2v_amd import inference
    res = {}
    for mode in ("host", "device"):
        out = tmp_path / f"{mode}.npz"
        assert inference.main(["--face", clip[0], "--audio", clip[1], "--max_frames", "8", "--LNet_batch_size", "4",
                               "--landmarks", "--geometry", mode, "--outfile", str(out)]) == 0
        res[mode] = (json.loads(capsys.readouterr().out.strip().splitlines()[-1]), np.load(out))
    (mh, sh), (md, sd) = res["host"], res["device"]
    assert mh["geometry"] == "host" and md["geometry"] == "device" and mh["frames"] == md["frames"] == 8
    assert md["landmark_rejects"] == mh["landmark_rejects"] and md["landmark_misses"] == mh["landmark_misses"]
    assert md["landmarks"] == mh["landmarks"] == "2DFAN4 synthetic"
    a, b = sd["semantic"], sh["semantic"]
    assert a.shape == b.shape == (8, 262) and np.isfinite(a).all()
    assert GC.ulps(a[:, 257:], b[:, 257:]).max() <= 1
    assert np.array_equal(a[:, :257], b[:, :257])
    diff = np.abs(sd["frames"].astype(np.int16) - sh["frames"].astype(np.int16))
    print(f"--geometry device: {int((diff != 0).sum())} of {diff.size} frame values differ from the host route's "
          f"(max {int(diff.max())}); {md['landmark_rejects']} rejected fits")
    assert diff.max() <= 1
