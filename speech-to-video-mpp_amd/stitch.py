"""The STIT reference stitch of datagen (inference.py:341-367) on the device: the names and signatures of
futils/alignment_stit.py, with device tensors where the reference has PIL images.

Per frame the reference takes the 68 landmarks of the stabilised frame, builds an FFHQ-style rotated square
around eyes and mouth (compute_transform, alignment_stit.py:116-146), resamples that square out of the
stabilised frame (crop_image: Pillow QUAD + BILINEAR, :68-114) and pastes it back with the inverse
perspective transform over the original crop (paste_image, :14-18, coefficients from
calc_alignment_coefficients, :199-209).  Inside the quad the networks then see the twice-resampled
stabilised face, outside it the original pixels.

The geometry (float64 NumPy, operation for operation as the reference, so that coefficients agree to the
bit where the host's LAPACK does) stays on the host; all pixels move in two launches per batch:
s2v_pil_transform_quad and s2v_pil_perspective_paste (csrc/stitch.hip), Pillow's arithmetic bit for bit.
There is no CPU path: frames are uint8 HWC device tensors.
"""
from __future__ import annotations

import numpy as np
import torch

from . import post
from ._lib import check

__all__ = ["compute_transform", "crop_faces", "crop_faces_by_quads", "crop_image", "calc_alignment_coefficients",
           "paste_image", "paste_images", "face_quads", "quad_coefficients", "crop_box", "gaussian_filter1d", "Stitcher"]


# ----------------------------------------------------------------------------- host geometry
def compute_transform(lm, predictor=None, detector=None, scale=1.0, fa=None):
    """alignment_stit.py:116-146: 68 landmarks [68, 2] -> (c, x, y): centre and the two half-axes of the
    oriented crop square.  ``predictor`` / ``detector`` / ``fa`` are unused, as in the reference."""
    lm = np.asarray(lm)
    eye_left = np.mean(lm[36:42], axis=0)
    eye_right = np.mean(lm[42:48], axis=0)
    eye_avg = (eye_left + eye_right) * 0.5
    eye_to_eye = eye_right - eye_left
    mouth_avg = (lm[48] + lm[54]) * 0.5            # the outer mouth's corners: lm_mouth_outer[0], [6]
    eye_to_mouth = mouth_avg - eye_avg
    x = eye_to_eye - np.flipud(eye_to_mouth) * [-1, 1]
    x /= np.hypot(*x)
    x *= max(np.hypot(*eye_to_eye) * 2.0, np.hypot(*eye_to_mouth) * 1.8)
    x *= scale
    y = np.flipud(x) * [-1, 1]
    c = eye_avg + eye_to_mouth * 0.1
    return c, x, y


def gaussian_filter1d(a, sigma, truncate=4.0):
    """scipy.ndimage.gaussian_filter1d(a, sigma, axis=0) with its defaults (order 0, mode 'reflect',
    truncate 4.0) in NumPy: scipy is no dependency of the package.  Sums in float64, result in the input's
    dtype, as scipy returns it."""
    dtype = np.asarray(a).dtype
    a = np.asarray(a, dtype=np.float64)
    lw = int(truncate * float(sigma) + 0.5)
    t = np.arange(-lw, lw + 1)
    k = np.exp(-0.5 / (float(sigma) * float(sigma)) * t ** 2)
    k = k / k.sum()
    pad = np.pad(a, [(lw, lw)] + [(0, 0)] * (a.ndim - 1), mode="symmetric")   # scipy's 'reflect': d c b a | a b c d
    out = np.zeros_like(a)
    for j in range(2 * lw + 1):
        out += k[j] * pad[j: j + a.shape[0]]
    return out.astype(dtype)


def make_quads(cs, xs, ys):
    """(nw, sw, se, ne) per frame, alignment_stit.py:180."""
    return np.stack([cs - xs - ys, cs - xs + ys, cs + xs + ys, cs + xs - ys], axis=1)


def crop_box(quad, output_size, width, height, name="frame"):
    """crop_image's host arithmetic (alignment_stit.py:69-92) for a width x height frame -> ((left, top,
    right, bottom), the quad relative to that box).  Raises ValueError where the reference cannot run: a
    non-finite corner, or the shrink branch (quad diagonal >= 4 x output_size, PIL.Image.ANTIALIAS)."""
    quad = np.array(quad)                          # a copy in the caller's dtype: the reference casts nothing
    if quad.shape != (4, 2):
        raise ValueError(f"crop_image: {name}: the quad must be [4, 2] (nw, sw, se, ne), got {quad.shape}")
    if not np.isfinite(quad).all():
        raise ValueError(f"crop_image: {name}: the quad has a non-finite corner (landmarks of a frame without a "
                         "face give 0/0)")
    x = (quad[3] - quad[1]) / 2
    qsize = np.hypot(*x) * 2
    shrink = int(np.floor(qsize / output_size * 0.5))
    if shrink > 1:
        raise ValueError(f"crop_image: {name}: quad diagonal {qsize:.1f} px is {qsize / output_size:.2f} x the output "
                         f"size {output_size}: the reference's shrink branch (>= 4 x) needs PIL.Image.ANTIALIAS, "
                         "which Pillow >= 10 lacks")
    border = max(int(np.rint(qsize * 0.1)), 3)
    crop = (int(np.floor(min(quad[:, 0]))), int(np.floor(min(quad[:, 1]))), int(np.ceil(max(quad[:, 0]))),
            int(np.ceil(max(quad[:, 1]))))
    crop = (max(crop[0] - border, 0), max(crop[1] - border, 0), min(crop[2] + border, width),
            min(crop[3] + border, height))
    if crop[2] - crop[0] < width or crop[3] - crop[1] < height:
        if crop[2] <= crop[0] or crop[3] <= crop[1]:
            raise ValueError(f"crop_image: {name}: the quad lies outside the {width}x{height} frame (crop box {crop})")
        quad -= crop[0:2]
        return crop, quad
    return (0, 0, width, height), quad


def quad_coefficients(quad, width, height):
    """Image.__transformer's QUAD branch: the corners (nw, sw, se, ne) of the source quad, as crop_image passes
    them ((quad + 0.5).flatten()), and the output size -> a0..a7, in Pillow's order of operations."""
    d = [float(v) for v in (np.asarray(quad) + 0.5).flatten()]      # Pillow reads each value as a C double
    nw, sw, se, ne = d[0:2], d[2:4], d[4:6], d[6:8]
    x0, y0 = nw
    As = 1.0 / width
    At = 1.0 / height
    return np.array([x0, (ne[0] - x0) * As, (sw[0] - x0) * At, (se[0] - sw[0] - ne[0] + x0) * As * At,
                     y0, (ne[1] - y0) * As, (sw[1] - y0) * At, (se[1] - sw[1] - ne[1] + y0) * As * At],
                    dtype=np.float64)


def quad_table(quads, output_size, width, height, names=None):
    """The kernel's table [n, 12] = (a0..a7, left, top, box width, box height) for n quads on width x height
    frames, and the crop boxes."""
    table = np.empty((len(quads), 12), dtype=np.float64)
    boxes = []
    for i, q in enumerate(quads):
        box, rel = crop_box(q, output_size, width, height, names[i] if names else f"frame {i}")
        table[i, :8] = quad_coefficients(rel, output_size, output_size)
        table[i, 8:] = (box[0], box[1], box[2] - box[0], box[3] - box[1])
        boxes.append(box)
    return table, boxes


def calc_alignment_coefficients(pa, pb):
    """alignment_stit.py:199-209: the eight PERSPECTIVE coefficients that map the points pa onto pb
    (inv(a^T a) a^T b in float64; the same NumPy operations in the same order, on ndarrays)."""
    matrix = []
    for p1, p2 in zip(pa, pb):
        matrix.append([p1[0], p1[1], 1, 0, 0, 0, -p2[0] * p1[0], -p2[0] * p1[1]])
        matrix.append([0, 0, 0, p1[0], p1[1], 1, -p2[1] * p1[0], -p2[1] * p1[1]])
    a = np.array(matrix, dtype=float)
    b = np.array(pb).reshape(8)
    res = np.dot(np.dot(np.linalg.inv(np.dot(a.T, a)), a.T), b)
    return np.array(res).reshape(8)


def square(image_size):
    """The corners of the crop the quad maps onto (inference.py:353)."""
    return [[0, 0], [0, image_size], [image_size, image_size], [image_size, 0]]


# ----------------------------------------------------------------------------- device launches
def _frames(x, what):
    if not (isinstance(x, torch.Tensor) and x.is_cuda and x.dtype == torch.uint8):
        raise RuntimeError(f"{what} must be a uint8 HIP tensor (the stitch has no CPU path)")
    if x.dim() == 3:
        x = x.unsqueeze(0)
    if x.dim() != 4 or x.shape[3] not in (3, 4):
        raise ValueError(f"{what} must be [H, W, C] or [n, H, W, C] with 3 or 4 channels, got {tuple(x.shape)}")
    return x


def transform_quad(frames, table, output_size, out=None):
    """One s2v_pil_transform_quad launch: frames uint8 [n, H, W, C] (row / image pitches free), table
    float64 [n, 12] (quad_table) -> uint8 [n, S, S, C]."""
    frames = _frames(frames, "transform_quad: frames")
    n, h, w, c, xrs, xis = post._hwc(frames)
    table = np.ascontiguousarray(table, dtype=np.float64)
    if table.shape != (n, 12) or not np.isfinite(table).all():
        raise ValueError(f"transform_quad: the table must be finite [{n}, 12], got {table.shape}")
    S = int(output_size)
    if out is None:
        out = torch.empty((n, S, S, c), dtype=torch.uint8, device=frames.device)
    on, oh, ow, oc, yrs, yis = post._hwc(_frames(out, "transform_quad: out"))
    if (on, oh, ow, oc) != (n, S, S, c):
        raise ValueError(f"transform_quad: out {tuple(out.shape)} != {(n, S, S, c)}")
    ctx = post._ctx(frames.device)
    tab = torch.from_numpy(table).to(frames.device)
    check(ctx.lib.s2v_pil_transform_quad(frames.data_ptr(), n, h, w, c, xrs, xis, tab.data_ptr(), out.data_ptr(), S, S,
                                         yrs, yis, ctx.stream), "s2v_pil_transform_quad")
    return out


def paste_images(coeffs, crops, targets, out=None):
    """paste_image for n frames in one s2v_pil_perspective_paste launch: coeffs float64 [n, 8], crops uint8
    [n, S, S, 3 | 4], targets uint8 [n, h, w, 3 | 4] -> RGB uint8 [n, h, w, 3] (``out``: given buffer, may be
    ``targets`` itself: in place)."""
    crops = _frames(crops, "paste_images: crops")
    targets = _frames(targets, "paste_images: targets")
    coeffs = np.ascontiguousarray(coeffs, dtype=np.float64).reshape(-1, 8)
    n, sh, sw, cc, crs, cis = post._hwc(crops)
    tn, h, w, tc, trs, tis = post._hwc(targets)
    if tn != n or coeffs.shape[0] != n:
        raise ValueError(f"paste_images: {n} crops, {tn} targets, {coeffs.shape[0]} coefficient rows")
    if not np.isfinite(coeffs).all():
        raise ValueError("paste_images: non-finite perspective coefficients")
    if out is None:
        out = torch.empty((n, h, w, 3), dtype=torch.uint8, device=crops.device)
    on, oh, ow, oc, yrs, yis = post._hwc(_frames(out, "paste_images: out"))
    if (on, oh, ow) != (n, h, w):
        raise ValueError(f"paste_images: out {tuple(out.shape)} != {(n, h, w, 3)}")
    ctx = post._ctx(crops.device)
    tab = torch.from_numpy(coeffs).to(crops.device)
    check(ctx.lib.s2v_pil_perspective_paste(crops.data_ptr(), n, sh, sw, cc, crs, cis, tab.data_ptr(),
                                            targets.data_ptr(), h, w, tc, trs, tis, out.data_ptr(), oc, yrs, yis,
                                            ctx.stream), "s2v_pil_perspective_paste")
    return out


def paste_image(inverse_transform, img, orig_image):
    """alignment_stit.py:14-18 followed by .convert('RGB') (inference.py:364): the crop ``img`` [S, S, 3 | 4]
    projected over ``orig_image`` [h, w, 3] -> uint8 [h, w, 3]."""
    return paste_images(np.asarray(inverse_transform, dtype=np.float64)[None], img[None], orig_image[None])[0]


def crop_image(frame, output_size, quad, enable_padding=False):
    """alignment_stit.py:68-114 for one frame uint8 [H, W, C] -> uint8 [S, S, C].  ``quad`` is not modified."""
    if enable_padding:
        raise NotImplementedError("crop_image: enable_padding is not on the inference path (it needs a gaussian "
                                  "filter and a median over the image)")
    frame = _frames(frame, "crop_image: frame")
    table, _ = quad_table([quad], output_size, frame.shape[2], frame.shape[1])
    return transform_quad(frame, table, output_size)[0]


def _files(files):
    """``files``: [(lm, frame), ...] or (lms [n, 68, 2], frames [n, H, W, C]) -> (lms list, frames [n, H, W, C],
    the frames as given)."""
    if isinstance(files, tuple) and len(files) == 2 and isinstance(files[1], torch.Tensor) and files[1].dim() == 4:
        lms = [None] * files[1].shape[0] if files[0] is None else list(files[0])
        return lms, files[1], list(files[1])
    lms = [lm for lm, _ in files]
    given = [f for _, f in files]
    if len({tuple(f.shape) for f in given}) != 1:
        raise ValueError("crop_faces: the frames of one call must share one shape (one launch)")
    return lms, torch.stack(given), given


def crop_faces_by_quads(IMAGE_SIZE, files, quads):
    """alignment_stit.py:188-196: -> (crops uint8 [n, S, S, C] from one launch, the frames as given)."""
    _, frames, given = _files(files)
    frames = _frames(frames, "crop_faces: frames")
    if len(quads) != frames.shape[0]:
        raise ValueError(f"crop_faces: {len(quads)} quads for {frames.shape[0]} frames")
    table, _ = quad_table(quads, IMAGE_SIZE, frames.shape[2], frames.shape[1])
    return transform_quad(frames, table, IMAGE_SIZE), given


def face_quads(lms, scale=1.0, center_sigma=0.0, xy_sigma=0.0):
    """crop_faces' host part (alignment_stit.py:162-181): the landmarks of n frames -> a list of n quads [4, 2]."""
    cs, xs, ys = [], [], []
    for lm in lms:
        c, x, y = compute_transform(lm, scale=scale)
        cs.append(c)
        xs.append(x)
        ys.append(y)
    cs, xs, ys = np.stack(cs), np.stack(xs), np.stack(ys)
    if center_sigma != 0:
        cs = gaussian_filter1d(cs, center_sigma)
    if xy_sigma != 0:
        xs = gaussian_filter1d(xs, xy_sigma)
        ys = gaussian_filter1d(ys, xy_sigma)
    return list(make_quads(cs, xs, ys))


def crop_faces(IMAGE_SIZE, files, scale, center_sigma=0.0, xy_sigma=0.0, use_fa=False, fa=None):
    """alignment_stit.py:149-185: -> (crops uint8 [n, S, S, C], the frames, quads: a list of [4, 2])."""
    lms, _, _ = _files(files)
    quads = face_quads(lms, scale, center_sigma, xy_sigma)
    crops, orig_images = crop_faces_by_quads(IMAGE_SIZE, files, quads)
    return crops, orig_images, quads


# ----------------------------------------------------------------------------- datagen's construction
class Stitcher:
    """datagen's reference construction (inference.py:348-364) as one object: landmarks of the stabilised
    references -> quads -> crops -> inverse coefficients -> paste over the resized original crops.

    ``keypoint_extractor``: a face3d.KeypointExtractor (any object with ``first_faces(frames)`` giving [68, 2]
    points per frame, all -1 without a face).  A frame without a face reuses the previous frame's points
    (extract_kp_videos.py:30-33), also across calls: the last points are kept until ``reset()``.  ``misses``
    counts the frames without a face that this object saw; the extractor keeps a counter of its own
    (``KeypointExtractor.misses``), which also counts frames it was given by other callers."""

    def __init__(self, keypoint_extractor, image_size=256, scale=1.0):
        self.kp = keypoint_extractor
        self.image_size = int(image_size)
        self.scale = scale
        self.misses = 0
        self.frames = 0
        self._last = None

    def reset(self):
        """Forget the last landmarks (a new clip)."""
        self._last = None

    def landmarks(self, frames):
        """frames uint8 [b, h, w, 3] -> [b, 68, 2] with the reuse rule applied."""
        out = []
        for kp in self.kp.first_faces(frames):
            kp = np.asarray(kp)
            if np.mean(kp) == -1:
                self.misses += 1
                if self._last is not None:
                    kp = self._last
            self._last = kp
            out.append(kp)
        self.frames += len(out)
        return np.stack(out)

    @torch.no_grad()
    def __call__(self, ref_u8: torch.Tensor, base_u8: torch.Tensor) -> torch.Tensor:
        """ref_u8 uint8 [b, 3, h, w]: the stabilised (possibly enhanced) references; base_u8 uint8 [b, h, w, 3]:
        the resized original crops (inference.py:361) -> the stitched references uint8 [b, 3, h, w]."""
        b = ref_u8.shape[0]
        if base_u8.shape[0] != b or base_u8.shape[3] != 3:
            raise ValueError(f"Stitcher: {b} references, base {tuple(base_u8.shape)}")
        # the reference hands the landmark detector the stabilised frames in the channel order they are
        # stored in (inference.py:349 wraps its arrays unchanged as PIL images), and so does this.  The stored
        # orders differ: the reference's frames are BGR, ref_u8 is RGB (trans_image's order), so FAN sees RGB
        # here where the reference's FAN sees BGR.  No flip is added on either side.
        frames = ref_u8.permute(0, 2, 3, 1).contiguous()
        first = self.frames
        lms = self.landmarks(frames)
        S = self.image_size
        try:
            crops, _, quads = crop_faces(S, (lms, frames), scale=self.scale, use_fa=True)
        except ValueError as e:
            raise ValueError(f"Stitcher: frames {first}..{first + b - 1} of the clip: {e}") from e
        inv = np.stack([calc_alignment_coefficients(q + 0.5, square(S)) for q in quads])
        pasted = paste_images(inv, crops, base_u8)
        return pasted.permute(0, 3, 1, 2).contiguous()
