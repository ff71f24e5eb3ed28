"""Inputs shared by the stitch tests and tests/golden/make_stitch_golden.py: the cases (images are
regenerated from their keys, so the fixture holds only recorded results), a synthetic 68-point face, and a
NumPy restatement of Pillow's BILINEAR transform, RGBA round trip and masked paste (test_stitch_host.py checks it
against Pillow itself where Pillow imports; the GPU tests use it for layouts the fixture has no case for)."""
import numpy as np

from s2v_amd import synth


def image(key, h, w, c=3):
    """uint8 [h, w, c] noise: every bilinear weight matters."""
    return np.floor(synth.hash_array(f"stitch.{key}", (h, w, c), 0.0, 256.0)).clip(0, 255).astype(np.uint8)


def rotated_square(cx, cy, half, degrees):
    """(nw, sw, se, ne) as crop_faces builds them from a centre and the half-axis x (y = x turned by 90 degrees)."""
    t = np.deg2rad(degrees)
    c = np.array([cx, cy], dtype=np.float64)
    x = half * np.array([np.cos(t), np.sin(t)])
    y = np.flipud(x) * [-1, 1]
    return np.stack([c - x - y, c - x + y, c + x + y, c + x - y])


# name -> (frame width, frame height, output size, quad).  Frames are image(name, H, W).
QUAD_CASES = {
    "inside": (48, 40, 32, rotated_square(24.0, 20.0, 9.0, 20.0)),          # wholly inside the frame
    "topleft": (48, 40, 32, rotated_square(6.0, 5.0, 10.0, -15.0)),         # zero fill, crop box clipped at 0
    "botright": (48, 40, 32, rotated_square(43.0, 36.0, 11.0, 30.0)),       # xin >= size, clamped last row / column
    "aligned": (48, 40, 32, rotated_square(23.5, 19.5, 16.0, 0.0)),         # data on integer corners: dx = dy = 0
    "deep256": (256, 256, 256, rotated_square(130.0, 120.0, 42.0, 12.0)),   # crop offset != 0, ~3x upsample
    "wide256": (256, 256, 256, rotated_square(128.0, 128.0, 361.0, 5.0)),   # qsize 1021: floor(qsize / S * 0.5) == 1
}
SMALL = ("inside", "topleft", "botright", "aligned")       # also the batch of four in one launch
SHRINK_QUAD = (256, 256, 256, rotated_square(128.0, 128.0, 363.0, 5.0))     # qsize 1027, shrink == 2: must raise

# paste cases beyond the inverse of every quad case: name -> (target width, height, crop size, crop channels,
# the four source points pa that map onto the crop's square)
PASTE_CASES = {
    "trapezoid": (48, 40, 32, 3, np.array([[8.0, 6.0], [4.0, 34.0], [44.0, 30.0], [38.0, 10.0]])),   # a6, a7 far from 0
    "miss": (48, 40, 32, 3, rotated_square(224.0, 220.0, 9.0, 20.0)),       # projects outside: output == target
    "cover": (48, 40, 32, 3, rotated_square(24.0, 20.0, 40.0, 8.0)),        # covers the whole target
    "rgba": (48, 40, 32, 4, np.array([[8.0, 6.0], [4.0, 34.0], [44.0, 30.0], [38.0, 10.0]])),        # alpha in 0..255
}


def face_landmarks(cx, cy, size, degrees=0.0):
    """A synthetic 68-point face (iBUG order) of about ``size`` px around (cx, cy), turned by ``degrees``."""
    p = np.zeros((68, 2), dtype=np.float64)
    a = np.linspace(np.pi, 0.0, 17)
    p[0:17] = np.stack([0.5 * np.cos(a), 0.1 + 0.55 * np.sin(a)], 1)                       # chin
    p[17:22] = np.stack([np.linspace(-0.38, -0.1, 5), np.full(5, -0.3)], 1)                # brows
    p[22:27] = np.stack([np.linspace(0.1, 0.38, 5), np.full(5, -0.3)], 1)
    p[27:31] = np.stack([np.zeros(4), np.linspace(-0.18, 0.05, 4)], 1)                     # nose
    p[31:36] = np.stack([np.linspace(-0.1, 0.1, 5), np.full(5, 0.12)], 1)
    e = np.arange(6) * (np.pi / 3)
    p[36:42] = np.stack([-0.22 - 0.08 * np.cos(e), -0.17 - 0.035 * np.sin(e)], 1)          # eyes
    p[42:48] = np.stack([0.22 - 0.08 * np.cos(e), -0.17 - 0.035 * np.sin(e)], 1)
    m = np.arange(12) * (np.pi / 6)
    p[48:60] = np.stack([-0.17 * np.cos(m), 0.3 - 0.07 * np.sin(m)], 1)                    # mouth: 48 left, 54 right
    n = np.arange(8) * (np.pi / 4)
    p[60:68] = np.stack([-0.11 * np.cos(n), 0.3 - 0.03 * np.sin(n)], 1)
    t = np.deg2rad(degrees)
    rot = np.array([[np.cos(t), -np.sin(t)], [np.sin(t), np.cos(t)]])
    return p @ rot.T * size + [cx, cy]


# compute_transform: landmark sets by name
LANDMARKS = {
    "centred": face_landmarks(128.0, 130.0, 150.0, 0.0),
    "corner": face_landmarks(30.0, 25.0, 120.0, -11.0),
    "small": face_landmarks(150.0, 90.0, 48.0, 17.0),
}

# crop_faces with smoothing: 6 frames of SMOOTH_HW, a face that drifts and turns
SMOOTH_HW = (64, 64)
SMOOTH_SIZE = 32
SMOOTH_SIGMAS = (1.5, 1.0)                        # center_sigma, xy_sigma
SMOOTH_LMS = np.stack([face_landmarks(30.0 + 1.7 * i + (i % 2) * 2.5, 33.0 - 0.9 * i, 30.0 + 1.3 * (i % 3), 3.0 * i - 6.0)
                       for i in range(6)])

# Stitcher: 3 frames; the middle one has no face and reuses its predecessor's points
STITCH_HW = (64, 64)
STITCH_SIZE = 64
STITCH_LMS = (face_landmarks(31.0, 33.0, 34.0, 6.0), None, face_landmarks(35.0, 30.0, 30.0, -9.0))


def stitch_inputs():
    """(stabilised references uint8 [3, H, W, 3], resized original crops uint8 [3, S, S, 3])."""
    h, w = STITCH_HW
    ref = np.stack([image(f"stitcher.ref{i}", h, w) for i in range(3)])
    base = np.stack([image(f"stitcher.base{i}", STITCH_SIZE, STITCH_SIZE) for i in range(3)])
    return ref, base


class CannedDetector:
    """get_landmarks_from_batch over a fixed list: per frame [points [68, 2]] or None (no face), in call order."""

    def __init__(self, lms):
        self.lms = list(lms)
        self.k = 0

    def get_landmarks_from_batch(self, batch):
        out = []
        for _ in range(len(batch)):
            lm = self.lms[self.k % len(self.lms)]
            self.k += 1
            out.append(None if lm is None else [np.asarray(lm, dtype=np.float32)])
        return out


# ----------------------------------------------------------------------------- Pillow's rule in NumPy
def pil_bilinear(src, xin, yin):
    """Pillow's BILINEAR transform filter (libImaging/Geometry.c) on a uint8 [h, w, c] image at the float64
    source coordinates (xin, yin): zero outside [0, w) x [0, h), neighbours clamped, (UINT8) truncation."""
    h, w, _ = src.shape
    valid = (xin >= 0.0) & (xin < w) & (yin >= 0.0) & (yin < h)
    xs = np.where(valid, xin, 0.5) - 0.5
    ys = np.where(valid, yin, 0.5) - 0.5
    x = np.floor(xs).astype(np.int64)
    y = np.floor(ys).astype(np.int64)
    dx = (xs - x)[..., None]
    dy = (ys - y)[..., None]
    x0, x1 = np.clip(x, 0, w - 1), np.clip(x + 1, 0, w - 1)
    s = src.astype(np.float64)
    a, b = s[np.clip(y, 0, h - 1), x0], s[np.clip(y, 0, h - 1), x1]
    v1 = a + (b - a) * dx
    a, b = s[np.minimum(y + 1, h - 1), x0], s[np.minimum(y + 1, h - 1), x1]
    v2 = np.where((y + 1 < h)[..., None], a + (b - a) * dx, v1)
    out = (v1 + (v2 - v1) * dy).astype(np.int64).astype(np.uint8)
    out[~valid] = 0
    return out


def pil_quad(src, a, size):
    """Image.transform((size, size), QUAD, ..., BILINEAR) of ``src`` given the eight coefficients a0..a7."""
    xx = np.arange(size)[None, :] + 0.5
    yy = np.arange(size)[:, None] + 0.5
    xin = a[0] + a[1] * xx + a[2] * yy + a[3] * xx * yy
    yin = a[4] + a[5] * xx + a[6] * yy + a[7] * xx * yy
    return pil_bilinear(src, xin, yin)


def _muldiv255(a, b):
    t = a.astype(np.int64) * b + 128
    return ((t >> 8) + t) >> 8


def pil_paste(crop, a, target):
    """paste_image + convert('RGB') (alignment_stit.py:14-18): crop uint8 [s, s, 3 | 4] under Image.transform(
    PERSPECTIVE, BILINEAR) with the eight coefficients ``a``, through Pillow's premultiplied RGBa round trip, then
    paste(projected, mask=projected) over target uint8 [h, w, 3] -> uint8 [h, w, 3]."""
    h, w, _ = target.shape
    if crop.shape[2] == 3:
        crop = np.concatenate([crop, np.full(crop.shape[:2] + (1,), 255, np.uint8)], 2)
    pm = crop.copy()
    pm[..., :3] = _muldiv255(crop[..., :3], crop[..., 3:4].astype(np.int64))            # RGBA -> RGBa
    xx = np.arange(w)[None, :] + 0.5
    yy = np.arange(h)[:, None] + 0.5
    den = a[6] * xx + a[7] * yy + 1
    p = pil_bilinear(pm, (a[0] * xx + a[1] * yy + a[2]) / den, (a[3] * xx + a[4] * yy + a[5]) / den)
    al = p[..., 3:4].astype(np.int64)
    rgb = p[..., :3].astype(np.int64)
    un = np.where((al == 255) | (al == 0), rgb, np.minimum((255 * rgb) // np.maximum(al, 1), 255))   # RGBa -> RGBA
    t = target.astype(np.int64) * (255 - al) + un * al + 128                           # BLEND8
    return (((t >> 8) + t) >> 8).astype(np.uint8)
