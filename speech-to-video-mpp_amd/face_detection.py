"""S3FD face detection and the face_detect box stage on the device: drop-ins for

    third_part/face_detection/detection/sfd/sfd_detector.py:16-59   SFDDetector
    third_part/face_detection/api.py:17-79                          LandmarksType, FaceAlignment
    futils/inference_utils.py:101-148                               get_smoothened_boxes, face_detect

    from s2v_amd import face_detection
    detector = face_detection.FaceAlignment(face_detection.LandmarksType._2D, flip_input=False, device='cuda:0')
    results = face_detection.face_detect(full_frames, pads=args.pads, nosmooth=args.nosmooth,
                                         jaw_correction=True, batch_size=args.face_det_batch_size,
                                         detector=detector)          # inference.py:357

On the device: the channel flip + mean subtraction of a batch of uint8 frames (s2v_u8_mean_nhwc4),
the S3FD network (models.S3FD: VGG-16 convs, max pools, s2v_l2norm_nhwc, fused heads) and
batch_detect's softmax + 0.05 threshold + prior decode over all six levels of the whole batch
(s2v_s3fd_decode).  One device -> host copy per batch brings the per-image counts and candidate rows;
the NMS over those few rows and the box arithmetic stay on the host, as in the reference.  With
SFDDetector(nms="device") (opt-in) the NMS runs on the device too (face.nms_device over s2v_nms, with score >
0.5 as its pre-filter) and the copy brings only the kept rows; among equal scores it takes the larger position
index first, where the reference leaves the order to NumPy's unstable sort.

The 68 landmarks of a face (face_alignment's get_landmarks_from_image / get_landmarks_from_batch, which
third_part/face3d/extract_kp_videos.py:15-57 calls) run on the device as well: utils.crop of every detected
face of a batch in one launch (s2v_fan_crop), the FAN network (models.FAN) and get_preds_fromhm's argmax
and quarter-pixel step (s2v_fan_peaks); one device -> host copy per batch brings the 68 heatmap points per
face, and their map back to frame coordinates (utils.transform's float32 matrix and .int()) stays on the
host, as the reference computes it.  With get_landmarks_from_batch(on_device=True) (opt-in) that map runs on
the device too (s2v_fan_landmarks over the host's inverse matrices, uploaded with the crop table) and the
points stay there.

Per-image equivalence with the reference's batched post-processing.  batch_detect (detect.py:77-92)
collects the UNION over the batch of the positions whose score passes 0.05 in any image, once per
hit, and evaluates every image at every collected position; SFDDetector.detect_from_batch then runs
nms(0.3) per image over all those rows and keeps score > 0.5.  Compared with an image's OWN
candidates (positions passing 0.05 in that image), the rows the union adds to an image score <= 0.05
there; in the score-ordered greedy NMS they come after every own candidate, so they suppress
nothing above them.  Repeated rows of one position have IoU 1 and suppress each other, leaving the
first.  All the added rows are then dropped by the > 0.5 filter.  So NMS over an image's own
candidates followed by > 0.5 gives the same kept list, in the same (descending score) order.
"""
from __future__ import annotations

import ctypes
import os
from enum import Enum

import numpy as np
import torch

from . import post
from ._lib import check
from .face import NMS_OK, nms_device, nms_mode, py_cpu_nms
from .ops import NHWC

MEANS = (104.0, 117.0, 123.0)           # detect.py:59, applied to the channels as the detector gets them
SCORE_THRESH = 0.05                     # detect.py:82
NMS_THRESH = 0.3                        # sfd_detector.py:43
KEEP_THRESH = 0.5                       # sfd_detector.py:45


class LandmarksType(Enum):
    """api.py:17-27."""
    _2D = 1
    _2halfD = 2
    _3D = 3


def _batch(images, device) -> torch.Tensor:
    t = images if isinstance(images, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(images))
    if t.dim() == 3:
        t = t.unsqueeze(0)
    if t.dtype != torch.uint8 or t.dim() != 4 or t.shape[3] != 3:
        raise TypeError(f"expected uint8 [B,H,W,3] frames, got {tuple(t.shape)} {t.dtype}")
    return t.to(device).contiguous()


def nms_keep(rows: np.ndarray):
    """sfd_detector.py:43-45 on one image's candidate rows [K,5]: nms(0.3), then score > 0.5."""
    if len(rows) == 0:
        return []
    kept = rows[py_cpu_nms(rows, NMS_THRESH), :]
    return [x for x in kept if x[-1] > KEEP_THRESH]


class SFDDetector:
    """sfd_detector.py:16-59 on the device.  ``net``: an s2v_amd.models.S3FD; without it the weights
    load from ``path_to_detector`` (strict).  Nothing is ever downloaded: a missing file is an error.
    ``nms``: "host" (nms_keep, the default), "device" (nms_device; an image with more than ``keep_max`` kept
    boxes, or one the kernel refuses, takes the host path alone) or None for S2V_NMS."""

    def __init__(self, device, path_to_detector=None, net=None, verbose=False, nms="host", keep_max=1024):
        from . import models
        self.nms = nms_mode(nms)
        self.keep_max = int(keep_max)
        self.device = torch.device(device)
        self.verbose = verbose
        if net is None:
            if not path_to_detector or not os.path.isfile(path_to_detector):
                raise FileNotFoundError(f"SFDDetector: no S3FD weights at {path_to_detector!r} (pass net= or a path)")
            net = models.load_s3fd(path_to_detector)
        self.face_detector = net.eval()
        self._cand = None

    def head_maps(self, images, flip=False):
        """uint8 [B,H,W,3] frames (host or device) -> the six fused head maps of the batch."""
        t = _batch(images, self.device)
        b, h, w, _ = t.shape
        from .models import s3fd_arch
        s3fd_arch.level_sizes(h, w)
        x4 = NHWC.empty(b, h, w, 4, self.device)
        ctx = post._ctx(self.device)
        mean = (ctypes.c_float * 3)(*MEANS)
        check(ctx.lib.s2v_u8_mean_nhwc4(t.data_ptr(), b, h * w, mean, 1 if flip else 0, x4.ptr, ctx.stream),
              "s2v_u8_mean_nhwc4")
        maps, _ = self.face_detector.head_maps(x4)
        return maps

    def candidates(self, maps):
        """Per image, the positions whose score > 0.05 as float32 rows [K,6] (position index bits, x1,
        y1, x2, y2, score) ordered by position index (level, row, column: batch_detect's order).  One
        device -> host copy of the counts and the candidate buffer."""
        n = maps[0].n
        P = sum(m.h * m.w for m in maps)
        if self._cand is None or self._cand.numel() < n * (P * 8 + 1):
            self._cand = torch.empty(n * (P * 8 + 1), device=self.device)
        buf = self._cand[: n * (P * 8 + 1)]
        count, cand = buf[:n], buf[n:]                      # counts (int bits) in front of the rows: one copy
        ctx = post._ctx(self.device)
        heads = (ctypes.c_void_p * 6)(*[m.ptr for m in maps])
        hs = (ctypes.c_int * 6)(*[m.h for m in maps])
        ws = (ctypes.c_int * 6)(*[m.w for m in maps])
        check(ctx.lib.s2v_s3fd_decode(heads, hs, ws, maps[0].cs, n, SCORE_THRESH, cand.data_ptr(), count.data_ptr(),
                                      P, ctx.stream), "s2v_s3fd_decode")
        host = buf.cpu().numpy()
        counts = host[:n].view(np.int32)
        rows = host[n:].reshape(n, P, 8)
        out = []
        for i in range(n):
            r = rows[i, : int(counts[i]), :6]
            out.append(r[np.argsort(r[:, 0].view(np.int32), kind="stable")].copy())
        return out

    @torch.no_grad()
    def detect_from_batch(self, images, flip=False):
        """-> per image, the list of kept [x1, y1, x2, y2, score] float32 rows (sfd_detector.py:41-47).
        ``flip``: reverse the channel order on the device first (FaceAlignment's images[..., ::-1])."""
        maps = self.head_maps(images, flip)
        if self.nms == "device":
            return self.detect_device(maps)
        return [nms_keep(r[:, 1:6]) for r in self.candidates(maps)]

    def decode(self, maps):
        """s2v_s3fd_decode -> (cand float32 [n * P * 8], count [n] int32 bits, n, P) on the device: the rows
        of the positions whose score > 0.05, in slot order (nms_device's input)."""
        n = maps[0].n
        P = sum(m.h * m.w for m in maps)
        if self._cand is None or self._cand.numel() < n * (P * 8 + 1):
            self._cand = torch.empty(n * (P * 8 + 1), device=self.device)
        buf = self._cand[: n * (P * 8 + 1)]
        count, cand = buf[:n], buf[n:]
        ctx = post._ctx(self.device)
        heads = (ctypes.c_void_p * 6)(*[m.ptr for m in maps])
        hs = (ctypes.c_int * 6)(*[m.h for m in maps])
        ws = (ctypes.c_int * 6)(*[m.w for m in maps])
        check(ctx.lib.s2v_s3fd_decode(heads, hs, ws, maps[0].cs, n, SCORE_THRESH, cand.data_ptr(), count.data_ptr(),
                                      P, ctx.stream), "s2v_s3fd_decode")
        return cand, count, n, P

    def detect_device(self, maps):
        """detect_from_batch's lists with the NMS on the device: nms(0.3) over the rows with score > 0.5 (a
        row at or below 0.5 comes after every row above it, suppresses none of them and is dropped after the
        NMS anyway).  One device -> host copy of the kept rows."""
        cand, count, n, P = self.decode(maps)
        res = nms_device(cand, count, n, P, 8, NMS_THRESH, min_score=KEEP_THRESH, keep_max=self.keep_max)
        host, out = None, []
        for i, (rows, status) in enumerate(res):
            if status != NMS_OK:
                host = self.candidates(maps) if host is None else host
                out.append(nms_keep(host[i][:, 1:6]))
            else:
                out.append(list(rows[:, 1:6]))
        return out

    def detect_from_image(self, img):
        """sfd_detector.py:31-39 for an image array / tensor [H,W,3]."""
        return self.detect_from_batch(_batch(img, self.device))[0]

    @property
    def reference_scale(self):
        return 195

    @property
    def reference_x_shift(self):
        return 0

    @property
    def reference_y_shift(self):
        return 0


# ----------------------------------------------------------------------------- FAN landmarks
FAN_RESOLUTION = 256.0                  # utils.crop's default resolution: the network input side
HEATMAP_SIZE = 64                       # the heatmaps' side at that input (s2v_fan_peaks takes no other)
# The glue between the detector and the network, get_landmarks_from_image, lives in the face-alignment
# 1.3.5 package, which is not part of the reference tree.  It adds two facts that stay parity-unpinned
# (no reference code or fixture pins them); everything else here restates reference code:
CENTER_Y_SHIFT = 0.12                   # the box centre is moved up by this fraction of the box height
HEATMAP_STACK = -1                      # the last stack's heatmaps are used
# utils.shuffle_lr's default pairs (utils.py:224-228): landmark k of a flipped face is landmark FLIP_PAIRS[k]
FLIP_PAIRS = (16, 15, 14, 13, 12, 11, 10, 9, 8, 7, 6, 5, 4, 3, 2, 1, 0, 26, 25, 24, 23, 22, 21, 20, 19, 18, 17, 27, 28,
              29, 30, 35, 34, 33, 32, 31, 45, 44, 43, 42, 47, 46, 39, 38, 37, 36, 41, 40, 54, 53, 52, 51, 50, 49, 48,
              59, 58, 57, 56, 55, 64, 63, 62, 61, 60, 67, 66, 65)


def transform_matrix(center, scale, resolution, invert=False) -> torch.Tensor:
    """The 3x3 float32 matrix of utils.transform (utils.py:77-85): ``center`` a float32 tensor (x, y),
    ``scale`` a Python float; torch.inverse when ``invert``."""
    h = 200.0 * scale
    t = torch.eye(3)
    t[0, 0] = resolution / h
    t[1, 1] = resolution / h
    t[0, 2] = resolution * (-center[0] / h + 0.5)
    t[1, 2] = resolution * (-center[1] / h + 0.5)
    return torch.inverse(t) if invert else t


def transform(point, center, scale, resolution, invert=False, matrix=None) -> torch.Tensor:
    """utils.transform (utils.py:56-89): the point through the matrix in torch float32, truncated by
    .int().  ``matrix``: transform_matrix(center, scale, resolution, invert) computed once for many points."""
    t = transform_matrix(center, scale, resolution, invert) if matrix is None else matrix
    pt = torch.ones(3)
    pt[0] = point[0]
    pt[1] = point[1]
    return torch.matmul(t, pt)[0:2].int()


def box_center_scale(d, reference_scale=195):
    """One detector row [x1, y1, x2, y2, ...] -> (center float32 tensor, scale float): the box centre with
    y moved up by CENTER_Y_SHIFT of the height, and (w + h) / reference_scale (sfd_detector.py:49-51)."""
    x1, y1, x2, y2 = (float(v) for v in d[:4])
    center = torch.tensor([x2 - (x2 - x1) / 2.0, y2 - (y2 - y1) / 2.0])
    center[1] = center[1] - (y2 - y1) * CENTER_Y_SHIFT
    return center, (x2 - x1 + y2 - y1) / reference_scale


def crop_window(center, scale, resolution=FAN_RESOLUTION):
    """utils.crop's window (utils.py:107-108): (ul.x, ul.y, br.x, br.y) ints in frame coordinates."""
    m = transform_matrix(center, scale, resolution, True)
    ul = transform([1, 1], center, scale, resolution, True, m)
    br = transform([resolution, resolution], center, scale, resolution, True, m)
    return int(ul[0]), int(ul[1]), int(br[0]), int(br[1])


def crop_table(frame_index, centers, scales, frame_hw) -> np.ndarray:
    """The per-face table of s2v_fan_crop: int32 [faces, 5] = (frame, ul.x, ul.y, br.x, br.y).  An empty
    window, or one that misses the frame (where utils.crop's slice assignment fails), raises ValueError."""
    H, W = frame_hw
    rows = []
    for f, c, s in zip(frame_index, centers, scales):
        ulx, uly, brx, bry = crop_window(c, s)
        if brx <= ulx or bry <= uly:
            raise ValueError(f"FAN crop: empty window ul=({ulx}, {uly}) br=({brx}, {bry}) for centre "
                             f"{[float(v) for v in c]} scale {s}")
        if min(brx, W) <= max(ulx, 0) or min(bry, H) <= max(uly, 0):
            raise ValueError(f"FAN crop: window ul=({ulx}, {uly}) br=({brx}, {bry}) misses the {W}x{H} frame")
        rows.append((int(f), ulx, uly, brx, bry))
    return np.asarray(rows, np.int32).reshape(-1, 5)


def preds_to_image(preds, center, scale, hm_size=64) -> torch.Tensor:
    """get_preds_fromhm's preds_orig (utils.py:163-168): each heatmap point [68, 2] through
    transform(.., hm_size, invert=True) -> float32 [68, 2] of integer values in frame coordinates."""
    m = transform_matrix(center, scale, hm_size, True)
    out = torch.zeros((len(preds), 2))
    for j in range(len(preds)):
        out[j] = transform(preds[j], center, scale, hm_size, True, m)
    return out


def back_map_matrix(center, scale, hm_size=64) -> np.ndarray:
    """Rows 0 and 1 of preds_to_image's matrix, transform_matrix(center, scale, hm_size, True), as float32 [6]:
    s2v_fan_landmarks takes the host's torch.inverse result as data."""
    return transform_matrix(center, scale, hm_size, True)[:2].reshape(6).numpy().copy()


class FaceAlignment:
    """api.py:46-79, plus the landmark half of face_alignment.FaceAlignment (get_landmarks_from_image /
    get_landmarks_from_batch) over the FAN network.  ``detector``: an SFDDetector; without it one is built
    from ``path_to_detector``.  ``fan``: an s2v_amd.models.FAN, or ``path_to_fan`` to load one; the
    landmark methods raise without either (nothing is downloaded)."""

    def __init__(self, landmarks_type, device="cuda", flip_input=False, face_detector="sfd", detector=None, *,
                 verbose=False, path_to_detector=None, fan=None, path_to_fan=None):
        if face_detector != "sfd":
            raise NotImplementedError("FaceAlignment: only the 'sfd' detector exists")
        self.device = device
        self.flip_input = flip_input
        self.landmarks_type = landmarks_type
        self.verbose = verbose
        self.face_detector = detector if detector is not None else SFDDetector(device, path_to_detector,
                                                                                        verbose=verbose)
        if fan is None and path_to_fan:
            if not os.path.isfile(path_to_fan):
                raise FileNotFoundError(f"FaceAlignment: no FAN weights at {path_to_fan!r}")
            from . import models
            fan = models.load_fan(path_to_fan)
        self.face_alignment_net = fan.eval() if fan is not None else None
        # flip_input's two index tables: the column order of the flipped crop / heatmap, and the landmark pairs
        self.flip_pairs = FLIP_PAIRS
        self.flip_columns = None            # None: reversed (utils.flip)
        self.fan_passes = 0                 # FAN forwards run so far

    # ------------------------------------------------------------------ landmarks
    def _flip_index(self, width, dev):
        cols = range(width - 1, -1, -1) if self.flip_columns is None else self.flip_columns(width)
        return torch.tensor(list(cols), dtype=torch.long, device=dev)

    def _fan(self, x4: NHWC) -> NHWC:
        self.fan_passes += 1
        return self.face_alignment_net.heatmaps(x4)[0][HEATMAP_STACK]

    def crops(self, frames: torch.Tensor, table: np.ndarray, dev_table: torch.Tensor | None = None) -> NHWC:
        """s2v_fan_crop: the 256x256 network inputs [faces, 256, 256, 4] of the table's faces.  ``dev_table``:
        the table in device memory already (face_tables), else it is uploaded here."""
        n, H, W, _ = frames.shape
        host = np.ascontiguousarray(table, np.int32)
        if dev_table is None:
            dev_table = torch.from_numpy(host).to(frames.device)
        size = int(FAN_RESOLUTION)
        x4 = NHWC.empty(len(host), size, size, 4, frames.device)
        ctx = post._ctx(frames.device)
        check(ctx.lib.s2v_fan_crop(frames.data_ptr(), n, H, W, dev_table.data_ptr(), host.ctypes.data, len(host), x4.ptr,
                                   ctx.stream), "s2v_fan_crop")
        return x4

    def peaks(self, hm: NHWC, on_device=False, k=None):
        """s2v_fan_peaks on heatmaps [faces, 64, 64, cs] -> (preds [faces, 68, 2], peak values [faces, 68])
        float32 host tensors: one device -> host copy.  ``on_device``: the two stay on the device (views of one
        buffer) and nothing is copied.  ``k``: the number of leading channels that are landmarks (default 68)."""
        from .models.fan_arch import NUM_LANDMARKS
        K = NUM_LANDMARKS if k is None else int(k)
        buf = torch.empty((hm.n, K * 3), device=hm.t.device)
        ctx = post._ctx(hm.t.device)
        check(ctx.lib.s2v_fan_peaks(hm.ptr, hm.n, hm.h, hm.w, K, hm.cs, buf.data_ptr(), buf.data_ptr() + 4 * hm.n * K * 2,
                                    ctx.stream), "s2v_fan_peaks")
        flat = buf.reshape(-1) if on_device else buf.cpu().reshape(-1)
        return flat[: hm.n * K * 2].reshape(hm.n, K, 2), flat[hm.n * K * 2:].reshape(hm.n, K)

    def face_tables(self, table: np.ndarray, mats: np.ndarray, device):
        """The crop table int32 [faces, 5] and the back-map matrices float32 [faces, 6] in one upload -> their
        two device views."""
        f = len(table)
        host = np.empty(f * 11, np.int32)
        host[: f * 5] = np.ascontiguousarray(table, np.int32).reshape(-1)
        host[f * 5:] = np.ascontiguousarray(mats, np.float32).reshape(-1).view(np.int32)
        dev = torch.from_numpy(host).to(device)
        return dev[: f * 5].view(f, 5), dev[f * 5:].view(torch.float32).view(f, 6)

    def landmarks_device(self, preds: torch.Tensor, mats: torch.Tensor) -> torch.Tensor:
        """s2v_fan_landmarks: device heatmap points [faces, k, 2] through the device matrices [faces, 6]
        (back_map_matrix) -> device float32 [faces, k, 2] of integer-valued frame coordinates: preds_to_image
        for every face in one launch."""
        f, k, _ = preds.shape
        if not (preds.is_cuda and preds.dtype == torch.float32 and preds.is_contiguous() and mats.is_cuda and
                mats.dtype == torch.float32 and mats.is_contiguous() and tuple(mats.shape) == (f, 6)):
            raise TypeError("landmarks_device: contiguous float32 device preds [faces, k, 2] and mats [faces, 6]")
        out = torch.empty_like(preds)
        if f == 0:
            return out
        ctx = post._ctx(preds.device)
        check(ctx.lib.s2v_fan_landmarks(preds.data_ptr(), mats.data_ptr(), f, k, out.data_ptr(), ctx.stream),
              "s2v_fan_landmarks")
        return out

    @torch.no_grad()
    def get_landmarks_from_batch(self, images, detected_faces=None, on_device=False):
        """images uint8 [B,H,W,3] RGB (host or device) -> per image None, or a list with one float32
        [68, 2] array of (x, y) frame coordinates per face, in the detector's order.  ``detected_faces``:
        per image a list of [x1, y1, x2, y2, ...] rows (else S3FD on the channel-flipped frames, as
        get_detections_for_batch).  Per face: centre / scale (box_center_scale), utils.crop, FAN,
        get_preds_fromhm on the last stack (flip_input: plus the flipped pass, utils.flip), preds_orig.
        ``on_device``: -> (device float32 [faces, 68, 2], the image index of every face as a host list), the
        same points with preds_orig on the device (s2v_fan_landmarks): the per-face inverse matrices go up
        with the crop table, nothing comes back and no per-point host work is done."""
        if self.face_alignment_net is None:
            raise RuntimeError("FaceAlignment: no FAN network (pass fan= or path_to_fan=)")
        t = _batch(images, self.device)
        if detected_faces is None:
            detected_faces = self.face_detector.detect_from_batch(t, flip=True)
        if len(detected_faces) != t.shape[0]:
            raise ValueError("get_landmarks_from_batch: one list of boxes per image")
        index = [i for i, dets in enumerate(detected_faces) for _ in dets]
        results = [None] * t.shape[0]
        if not index:
            if on_device:
                from .models.fan_arch import NUM_LANDMARKS
                return torch.empty((0, NUM_LANDMARKS, 2), device=t.device), index
            return results
        ref = self.face_detector.reference_scale
        cs = [box_center_scale(d, ref) for dets in detected_faces for d in dets]
        table = crop_table(index, [c for c, _ in cs], [s for _, s in cs], t.shape[1:3])
        dev_table = mats = None
        if on_device:
            dev_table, mats = self.face_tables(table, np.stack([back_map_matrix(c, s, HEATMAP_SIZE) for c, s in cs]),
                                               t.device)
        x4 = self.crops(t, table, dev_table)
        hm = self._fan(x4)
        if self.flip_input:
            # out += flip(net(flip(inp))[-1], is_label=True): columns reversed, landmark channels paired
            dev = hm.t.device
            xf = NHWC(x4.t.index_select(2, self._flip_index(x4.w, dev)).contiguous())
            hf = self._fan(xf)
            k = len(self.flip_pairs)
            back = hf.t[..., :k].index_select(2, self._flip_index(hf.w, dev))
            back = back.index_select(3, torch.tensor(list(self.flip_pairs), dtype=torch.long, device=dev))
            hm = NHWC((hm.t[..., :k] + back).contiguous())
        if on_device:
            if hm.h != HEATMAP_SIZE:
                raise ValueError(f"get_landmarks_from_batch: {hm.h}x{hm.w} heatmaps, the matrices are for {HEATMAP_SIZE}")
            return self.landmarks_device(self.peaks(hm, on_device=True)[0], mats), index
        preds, _ = self.peaks(hm)
        for f, (i, (c, s)) in enumerate(zip(index, cs)):
            pts = preds_to_image(preds[f], c, s, hm.h).numpy()
            results[i] = (results[i] or []) + [pts]
        return results

    def get_landmarks_from_image(self, image, detected_faces=None):
        """One uint8 [H,W,3] RGB image -> None without a face, else the list of [68, 2] arrays."""
        return self.get_landmarks_from_batch(_batch(image, self.device),
                                             None if detected_faces is None else [detected_faces])[0]

    def get_detections_for_batch(self, images):
        """images uint8 [B,H,W,3] -> per image (x1, y1, x2, y2) ints of the first kept box, or None."""
        detected_faces = self.face_detector.detect_from_batch(images, flip=True)
        results = []
        for d in detected_faces:
            if len(d) == 0:
                results.append(None)
                continue
            d = np.clip(d[0], 0, None)
            x1, y1, x2, y2 = map(int, d[:-1])
            results.append((x1, y1, x2, y2))
        return results


def get_smoothened_boxes(boxes, T):
    """inference_utils.py:101-108, in place on the caller's array (an integer array truncates every
    mean on assignment, and the tail windows read rows that are already smoothed)."""
    for i in range(len(boxes)):
        if i + T > len(boxes):
            window = boxes[len(boxes) - T:]
        else:
            window = boxes[i: i + T]
        boxes[i] = np.mean(window, axis=0)
    return boxes


def _shape_hw(image):
    return int(image.shape[0]), int(image.shape[1])


def face_detect(images, pads=(0, 20, 0, 0), nosmooth=False, jaw_correction=False, batch_size=4, detector=None):
    """inference_utils.py:110-148 -> [[crop, (y1, y2, x1, x2)], ...] per frame.  ``images``: a list of
    uint8 [H,W,3] frames or one [N,H,W,3] array / device tensor; ``detector``: anything with
    get_detections_for_batch (a FaceAlignment)."""
    if detector is None:
        detector = FaceAlignment(LandmarksType._2D, flip_input=False, device="cuda:0")
    while 1:
        predictions = []
        try:
            for i in range(0, len(images), batch_size):
                chunk = images[i:i + batch_size]
                if not isinstance(chunk, torch.Tensor):
                    chunk = np.array(chunk)
                predictions.extend(detector.get_detections_for_batch(chunk))
        except RuntimeError:
            if batch_size == 1:
                raise RuntimeError("Image too big to run face detection on GPU. Please use the --resize_factor argument")
            batch_size //= 2
            print("Recovering from OOM error; New batch size: {}".format(batch_size))
            continue
        break

    results = []
    pady1, pady2, padx1, padx2 = pads if jaw_correction else (0, 20, 0, 0)
    for rect, image in zip(predictions, images):
        if rect is None:
            raise ValueError("Face not detected! Ensure the video contains a face in all the frames.")
        h, w = _shape_hw(image)
        y1 = max(0, rect[1] - pady1)
        y2 = min(h, rect[3] + pady2)
        x1 = max(0, rect[0] - padx1)
        x2 = min(w, rect[2] + padx2)
        results.append([x1, y1, x2, y2])

    boxes = np.array(results)
    if not nosmooth:
        boxes = get_smoothened_boxes(boxes, T=5)
    return [[image[y1:y2, x1:x2], (y1, y2, x1, x2)] for image, (x1, y1, x2, y2) in zip(images, boxes)]
