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
the NMS over those few rows and the box arithmetic stay on the host, as in the reference.

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
from .face import py_cpu_nms
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
    load from ``path_to_detector`` (strict).  Nothing is ever downloaded: a missing file is an error."""

    def __init__(self, device, path_to_detector=None, net=None, verbose=False):
        from . import models
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
        return [nms_keep(r[:, 1:6]) for r in self.candidates(self.head_maps(images, flip))]

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


class FaceAlignment:
    """api.py:46-79 (the detector half: the FAN landmark network is not on the face_detect path).
    ``detector``: an SFDDetector; without it one is built from ``path_to_detector``."""

    def __init__(self, landmarks_type, device="cuda", flip_input=False, face_detector="sfd", detector=None, *,
                 verbose=False, path_to_detector=None):
        if face_detector != "sfd":
            raise NotImplementedError("FaceAlignment: only the 'sfd' detector exists")
        self.device = device
        self.flip_input = flip_input
        self.landmarks_type = landmarks_type
        self.verbose = verbose
        self.face_detector = detector if detector is not None else SFDDetector(device, path_to_detector,
                                                                                        verbose=verbose)

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
