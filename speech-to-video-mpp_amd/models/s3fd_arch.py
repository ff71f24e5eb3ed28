"""Parameter layout of the S3FD face detector (third_part/face_detection/detection/sfd/net_s3fd.py:
22-68), the network SFDDetector builds (sfd_detector.py:26) and FaceAlignment's default detector.

A VGG-16 trunk (conv1_1 .. conv5_3, fc6 / fc7 as convs), two extra stride-2 stages (conv6_*, conv7_*),
three L2Norm scale vectors and a class + box head per detection level.  The class only declares the
parameters under the reference attribute paths, so an ``s3fd.pth`` state_dict loads with strict=True.
"""
from __future__ import annotations

import torch
from torch import nn

# (name, cin, cout, kernel, stride, padding) in forward order
TRUNK = (
    ("conv1_1", 3, 64, 3, 1, 1), ("conv1_2", 64, 64, 3, 1, 1),
    ("conv2_1", 64, 128, 3, 1, 1), ("conv2_2", 128, 128, 3, 1, 1),
    ("conv3_1", 128, 256, 3, 1, 1), ("conv3_2", 256, 256, 3, 1, 1), ("conv3_3", 256, 256, 3, 1, 1),
    ("conv4_1", 256, 512, 3, 1, 1), ("conv4_2", 512, 512, 3, 1, 1), ("conv4_3", 512, 512, 3, 1, 1),
    ("conv5_1", 512, 512, 3, 1, 1), ("conv5_2", 512, 512, 3, 1, 1), ("conv5_3", 512, 512, 3, 1, 1),
    ("fc6", 512, 1024, 3, 1, 3), ("fc7", 1024, 1024, 1, 1, 0),
    ("conv6_1", 1024, 256, 1, 1, 0), ("conv6_2", 256, 512, 3, 2, 1),
    ("conv7_1", 512, 128, 1, 1, 0), ("conv7_2", 128, 256, 3, 2, 1),
)
# a 2x2 stride-2 max pool follows these trunk convs
POOL_AFTER = ("conv1_2", "conv2_2", "conv3_3", "conv4_3", "conv5_3")
# (name, channels, initial scale): the L2Norm of a detection source; it feeds the heads only
L2NORMS = (("conv3_3_norm", 256, 10.0), ("conv4_3_norm", 512, 8.0), ("conv5_3_norm", 512, 5.0))
L2NORM_EPS = 1e-10
# detection levels, stride 4 .. 128: (head prefix, trunk source, source channels, class logits)
LEVELS = (
    ("conv3_3_norm", "conv3_3", 256, 4), ("conv4_3_norm", "conv4_3", 512, 2), ("conv5_3_norm", "conv5_3", 512, 2),
    ("fc7", "fc7", 1024, 2), ("conv6_2", "conv6_2", 512, 2), ("conv7_2", "conv7_2", 256, 2),
)
MIN_SIZE = 2 ** len(POOL_AFTER)        # every pool halves a map that must be at least 2 wide


class _Scale(nn.Module):
    """L2Norm: one learned scale per channel."""

    def __init__(self, channels, scale):
        super().__init__()
        self.weight = nn.Parameter(torch.full((channels,), float(scale)))


class S3FDParams(nn.Module):
    def __init__(self):
        super().__init__()
        for name, cin, cout, k, s, p in TRUNK:
            setattr(self, name, nn.Conv2d(cin, cout, k, s, p))
        for name, ch, scale in L2NORMS:
            setattr(self, name, _Scale(ch, scale))
        for prefix, _, ch, nconf in LEVELS:
            setattr(self, prefix + "_mbox_conf", nn.Conv2d(ch, nconf, 3, 1, 1))
            setattr(self, prefix + "_mbox_loc", nn.Conv2d(ch, 4, 3, 1, 1))


def level_sizes(h: int, w: int):
    """(h, w) of the six detection levels for an h x w input."""
    if min(h, w) < MIN_SIZE:
        raise ValueError(f"S3FD: a {h}x{w} input is too small for the {len(POOL_AFTER)} poolings "
                         f"(both sides must be at least {MIN_SIZE})")
    sizes = {}
    for name, _, _, k, s, p in TRUNK:
        h, w = (h + 2 * p - k) // s + 1, (w + 2 * p - k) // s + 1
        sizes[name] = (h, w)
        if name in POOL_AFTER:
            h, w = h // 2, w // 2
    return [sizes[src] for _, src, _, _ in LEVELS]
