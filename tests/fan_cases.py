"""Inputs shared by the FAN tests and tests/golden/make_fan_golden.py: the recorded cases (frames and
weights are regenerated from their keys), and the bounds derived from the forward tolerance."""
import functools

import numpy as np

from s2v_amd import synth

FORWARD_RTOL = 1e-3        # per stack: max|d| <= 1e-3 * max(1, max|ref|), the detectors' bound (s3fd_cases.FORWARD_RTOL)
CHANNEL_STEP = 4           # the fixture keeps every fourth heatmap channel (and the forward case's last stack in full)

# forward: 2 x 128 x 128 (maps 32x32, the hourglass bottom level 2x2); full: one 256 x 256 crop (maps 64x64)
FORWARD = ("fan.forward", 2, 128, 128)
FULL = ("fan.full", 1, 256, 256)
# the stated centre / scale that map the full case's heatmap points back to frame coordinates
FULL_CENTER = (131.0, 117.5)
FULL_SCALE = 1.31

# crop: two 90 x 120 frames, six boxes (frame, x1, y1, x2, y2): inside the frame, over the left / top / right /
# bottom edge, and larger than the frame
CROP = ("fan.crop", 2, 90, 120)
# (utils.crop's window is about twice the box: 200 * (w + h) / 195 pixels wide)
CROP_BOXES = ((0, 45.2, 30.7, 83.1, 69.3), (1, 2.6, 30.3, 41.0, 68.9), (0, 50.5, 4.8, 87.2, 41.4),
              (1, 77.3, 28.2, 115.9, 66.0), (0, 40.9, 44.6, 78.4, 82.3), (1, -10.5, -25.1, 130.3, 110.8))
# glue: boxes [x1, y1, x2, y2, score] on the full case's frame (one inside, one over the corner)
GLUE_BOXES = ((38.4, 52.7, 201.3, 223.9, 0.99), (-21.5, -12.25, 118.0, 131.5, 0.97))


def frames(case):
    key, n, h, w = case
    return synth.sr_frame(key, n, h, w)


def net_input(case):
    """float32 [n,3,H,W] = frame / 255 as get_landmarks_from_image feeds the network."""
    return (frames(case).transpose(0, 3, 1, 2).astype(np.float32) / np.float32(255.0)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def state_dict():
    from s2v_amd.models.fan_arch import FANParams
    return synth.synth_torch_state_dict(FANParams(4), **synth.FAN_SYNTH)


def forward_eps(ref_max: float) -> float:
    return FORWARD_RTOL * max(1.0, float(ref_max))
