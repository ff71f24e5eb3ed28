"""Inputs shared by the geometry tests (test_geom_cases_host.py, test_geom_gpu.py), the contracts of
s2v_fan_landmarks, s2v_face3d_align and s2v_dnet_windows (include/s2v.h) restated in NumPy, and the existing
host routes they replace, packed the way the kernels' outputs are."""
import functools

import numpy as np
import torch

from helpers import FACE3D_LM3D, face3d_landmarks
from s2v_amd import synth

# ----------------------------------------------------------------------------- landmarks
HM = 64
# (centre x, centre y, scale): an integer centre with scale 0.32 * 4 (the inverse scales by 4: every quarter
# point lands exactly on an integer), the same with 0.32 * 2 (integers and halves), and a face whose window
# hangs over the frame's top-left corner (negative coordinates: truncation toward zero is not floor)
LANDMARK_FACES = ((120.0, 96.0, 1.28), (57.0, 43.0, 0.64), (20.3, 15.7, 1.1))


@functools.lru_cache(maxsize=None)
def odd_matrix_face():
    """A (centre x, centre y, scale) whose torch.inverse matrix has m[2][2] != 1 (LU leaves that in about a
    fifth of random faces): the first such of a seeded sequence, so the case holds wherever LU rounds."""
    from s2v_amd import face_detection as fd
    rng = np.random.default_rng(2)
    for _ in range(2000):
        cx, cy, s = float(rng.uniform(20, 400)), float(rng.uniform(20, 300)), float(rng.uniform(0.4, 2.5))
        if float(fd.transform_matrix(torch.tensor([cx, cy]), s, HM, True)[2, 2]) != 1.0:
            return cx, cy, s
    raise AssertionError("no face with m[2][2] != 1 among 2000")


def landmark_faces():
    return LANDMARK_FACES + (odd_matrix_face(),)


def landmark_preds(faces, k=68, key="geom.lm"):
    """float32 [faces, k, 2] heatmap points as s2v_fan_peaks writes them: position + 1 + step - 0.5 with the
    position in 0..63 and the step in (-0.25, 0, 0.25); the first points are the extremes 0.5 and 63.5."""
    pos = np.floor(synth.hash_array(key + ".pos", (faces, k, 2), 0.0, 64.0)).clip(0, 63)
    step = (np.floor(synth.hash_array(key + ".step", (faces, k, 2), 0.0, 3.0)).clip(0, 2) - 1.0) * 0.25
    inner = ((pos > 0) & (pos < 63)).all(-1, keepdims=True)          # a border maximum takes no step
    p = (pos + 1.0 + step * inner - 0.5).astype(np.float32)
    p[:, 0] = (0.5, 63.5)
    p[:, 1] = (63.5, 0.5)
    p[:, 2] = (0.5, 0.5)
    p[:, 3] = (63.5, 63.5)
    return p


def landmark_mats(faces):
    """float32 [faces, 6]: rows 0 and 1 of every face's inverse matrix, as the device route uploads them."""
    from s2v_amd import face_detection as fd
    return np.stack([fd.back_map_matrix(torch.tensor([cx, cy]), s, HM) for cx, cy, s in faces])


def landmarks_numpy(preds, mats):
    """s2v_fan_landmarks: v = (m0 x + m1 y) + m2 in float32, each step rounded, truncated toward zero."""
    p = np.asarray(preds, np.float32)
    m = np.asarray(mats, np.float32)[:, None, :]
    x, y = p[..., 0], p[..., 1]
    out = np.empty_like(p)
    for a in range(2):
        v = (m[..., 3 * a] * x + m[..., 3 * a + 1] * y).astype(np.float32) + m[..., 3 * a + 2]
        out[..., a] = np.trunc(v.astype(np.float32))
    return out


def landmarks_host(preds, faces):
    """The host route: face_detection.preds_to_image per face."""
    from s2v_amd import face_detection as fd
    return np.stack([fd.preds_to_image(torch.from_numpy(np.ascontiguousarray(p)), torch.tensor([cx, cy]), s, HM).numpy()
                     for p, (cx, cy, s) in zip(preds, faces)])


# ----------------------------------------------------------------------------- align
LM3D = FACE3D_LM3D
ALIGN_SIZES = ((240, 180), (1400, 1400))                  # (W, H)
# (eye distance px, centre x, centre y, roll deg) of the three plausible faces and of the one spread past the
# 11.5x downscale, per frame size; between them one frame without landmarks and one with all points equal.  No
# face sits on the frame's centre line unrolled: such a fit has t0 = w0 / 2 up to rounding, and left on an integer
ALIGN_FACES = {(240, 180): ((60.0, 113.0, 85.0, 0.0), (150.0, 110.0, 95.0, 4.0), (70.0, 140.0, 100.0, 20.0)),
               (1400, 1400): ((330.0, 688.0, 640.0, 0.0), (610.0, 520.0, 810.0, -7.0), (95.0, 1180.0, 240.0, 15.0))}
ALIGN_WIDE = {(240, 180): (1500.0, 120.0, 90.0, 0.0), (1400, 1400): (9000.0, 700.0, 700.0, 3.0)}
ALIGN_STATUS = (0, 0, 0, 1, 2, 2)


def align_landmarks(size):
    """float32 [6, 68, 2]: three faces, all -1, all points equal (an infinite or absurd scale), one too wide."""
    faces = face3d_landmarks(ALIGN_FACES[size] + (None,))
    equal = np.tile(np.array([[size[0] * 0.4 + 0.5, size[1] * 0.45 + 0.25]], np.float32), (68, 1))
    wide = face3d_landmarks((ALIGN_WIDE[size],))[0]
    return np.stack(faces + [equal, wide]).astype(np.float32)


def align_fit_numpy(p5, W, H, pinv, target=224.0, rescale=102.0):
    """Step 3 of s2v_face3d_align in float64 -> (usable, box or None, trans float32 [5], the four values before
    truncation)."""
    with np.errstate(all="ignore"):
        p5 = np.asarray(p5, np.float64)
        kx, ky = np.zeros(4), np.zeros(4)
        for r in range(4):
            for j in range(5):
                kx[r] = kx[r] + pinv[r, j] * p5[j, 0]
                ky[r] = ky[r] + pinv[r, j] * p5[j, 1]
        n1 = np.sqrt((kx[0] * kx[0] + kx[1] * kx[1]) + kx[2] * kx[2])
        n2 = np.sqrt((ky[0] * ky[0] + ky[1] * ky[1]) + ky[2] * ky[2])
        s = np.float64(rescale) / ((n1 + n2) / 2.0)
        t0, t1 = kx[3], ky[3]
        trans = np.array([W, H, s, t0, t1], np.float64).astype(np.float32)
        wd, hd = W * s, H * s
        fits = lambda v: bool(-2.0 ** 31 < v < 2.0 ** 31)  # noqa: E731  (False for NaN)
        if not (fits(wd) and fits(hd)):
            return False, None, trans, (wd, hd, np.nan, np.nan)
        w, h = int(wd), int(hd)
        if w <= 0 or h <= 0 or W / w > 11.5 or H / h > 11.5:
            return False, None, trans, (wd, hd, np.nan, np.nan)
        ld = (w / 2 - target / 2) + (t0 - W / 2) * s
        ud = (h / 2 - target / 2) + (H / 2 - t1) * s
        if not (fits(ld) and fits(ud)):
            return False, None, trans, (wd, hd, ld, ud)
        return True, (w, h, int(ld), int(ud)), trans, (wd, hd, ld, ud)


def align_numpy(lms, W, H, lm3d=LM3D):
    """s2v_face3d_align -> (params int32 [n, 4], trans float32 [n, 5], status int32 [n])."""
    from s2v_amd import face3d
    pinv, (dbox, dtrans) = face3d.pos_pinv(lm3d), face3d.default_fit(lm3d, W, H)
    params, trans, status = [], [], []
    for lm in np.asarray(lms, np.float32):
        ok, st = False, 1
        if not (lm == np.float32(-1)).all():
            x, y = lm[:, 0], (np.float32(H - 1) - lm[:, 1]).astype(np.float32)
            mean = lambda v, a, b: np.float32(np.float32(v[a] + v[b]) / np.float32(2))  # noqa: E731
            p5 = [(mean(x, 36, 39), mean(y, 36, 39)), (mean(x, 42, 45), mean(y, 42, 45)), (x[30], y[30]),
                  (x[48], y[48]), (x[54], y[54])]
            ok, box, tr, _ = align_fit_numpy(p5, W, H, pinv)
            st = 0 if ok else 2
        if not ok:
            box, tr = dbox, dtrans                          # the host's fit of the no-landmark points, as data
        params.append(box)
        trans.append(tr)
        status.append(st)
    return np.asarray(params, np.int32), np.stack(trans), np.asarray(status, np.int32)


def align_host(lms, W, H, lm3d=LM3D):
    """The host route: inference._usable_landmarks, then face3d.frame_landmarks + align_params per frame ->
    (params int32 [n, 4], trans float32 [n, 5] as Face3DExtractor.coeffs rounds them, status int32 [n], the four
    values before truncation [n, 4] float64 of the fit of the frame's own landmarks: NaN for a frame without
    landmarks, and where the host route raises before it gets there)."""
    from s2v_amd import face3d, inference
    lms = np.asarray(lms, np.float32)
    usable, _ = inference._usable_landmarks(lms, H, W, lm3d)
    params, trans, status, raw = [], [], [], []
    for before, lm in zip(lms, usable):
        none = np.mean(before) == -1
        status.append(1 if none else 2 if np.mean(lm) == -1 else 0)
        t, box, _ = face3d.align_params(W, H, face3d.frame_landmarks(lm, W, H, lm3d), lm3d)
        params.append(box)
        trans.append(np.array([float(v) for v in t], dtype=np.float32))
        values = [np.nan] * 4
        if not none:
            try:
                with np.errstate(all="ignore"):
                    t, box, _ = face3d.align_params(W, H, face3d.frame_landmarks(before, W, H, lm3d), lm3d)
                w0, h0, s, t0, t1 = (float(v) for v in t)
                values = [w0 * s, h0 * s, box[0] / 2 - 224.0 / 2 + (t0 - w0 / 2) * s,
                          box[1] / 2 - 224.0 / 2 + (h0 / 2 - t1) * s]
            except (ValueError, OverflowError):
                pass
        raw.append(values)
    return np.asarray(params, np.int32), np.stack(trans), np.asarray(status, np.int32), np.asarray(raw, np.float64)


def ulps(a, b):
    """Distance in float32 steps between two finite float32 arrays (0 between -0 and +0)."""
    def key(v):
        i = np.ascontiguousarray(v, np.float32).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7FFFFFFF), i)
    return np.abs(key(a) - key(b))


# ----------------------------------------------------------------------------- windows
def window_semantic(N):
    """float32 [N, 262].  A later frame repeats an earlier one in the columns the ratio's search compares
    (80:144, 224:227) with another column 259, one compared value being +0 in one and -0 in the other: N >= 10:
    frame 7 repeats frame 3, and frame 9 repeats it with column 259 = 0 (a ratio of exactly 0: row 70 stays
    unscaled); smaller clips: frame N - 1 repeats frame 1."""
    sem = synth.hash_array(f"geom.semantic.{N}", (N, 262), -1.0, 1.0).astype(np.float32)
    a, b = (3, 7) if N >= 10 else (1, N - 1)
    for cols in (slice(80, 144), slice(224, 227)):
        sem[b, cols] = sem[a, cols]
    sem[a, 85], sem[b, 85] = np.float32(0.0), np.float32(-0.0)
    sem[b, 259] = sem[a, 259] * np.float32(1.75) + np.float32(0.125)
    if N >= 10:
        for cols in (slice(80, 144), slice(224, 227)):
            sem[9, cols] = sem[a, cols]
        sem[9, 259] = 0.0
    return sem


WINDOW_CLIPS = (30, 5)


def window_ranges(N):
    return ((0, N), (3, 9)) if N >= 9 else ((0, N),)


def window_expression():
    return synth.hash_array("geom.expression", (64,), -1.0, 1.0).astype(np.float32)


def windows_numpy(sem, expression=None, one_shot=False, start=0, stop=None):
    """s2v_dnet_windows: the first-equal rule instead of find_crop_norm_ratio's argmin."""
    sem = np.asarray(sem, np.float32)
    N = sem.shape[0]
    stop = N if stop is None else stop
    cols = np.r_[80:144, 224:227, 254:257, 259:262]
    cmp = np.r_[80:144, 224:227]
    out = np.empty((stop - start, 73, 26), np.float32)
    for k, idx in enumerate(range(start, stop)):
        src = 0 if one_shot else idx
        j = next(j for j in range(N) if (sem[j, cmp] == sem[src, cmp]).all())
        with np.errstate(all="ignore"):
            ratio = np.float32(sem[src, 259] / sem[j, 259])
        frames = np.clip(np.arange(idx - 13, idx + 13), 0, N - 1)
        win = sem[frames][:, cols].T.copy()
        if ratio != 0:
            win[70] = win[70] * ratio
        if expression is not None:
            win[:64] = np.asarray(expression, np.float32)[:64, None]
        out[k] = win
    return out
