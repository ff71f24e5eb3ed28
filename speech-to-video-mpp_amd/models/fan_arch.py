"""Parameter layout of the FAN landmark network (third_part/face_detection/models.py:13-201): the
stacked-hourglass 2D-FAN-4 that face_alignment's FaceAlignment(LandmarksType._2D) runs.

Stem conv1 7x7/2 + bn1, ConvBlocks conv2 / conv3 / conv4, then ``num_modules`` stacks of
HourGlass(1, 4, 256) ``m{i}`` + ConvBlock ``top_m_{i}`` + ``conv_last{i}`` / ``bn_end{i}`` + the 68
heatmap conv ``l{i}``, with ``bl{i}`` / ``al{i}`` feeding the next stack.  The classes only declare the
parameters under the reference attribute paths, so a 2DFAN4 state_dict loads with strict=True.
"""
from __future__ import annotations

from torch import nn

NUM_LANDMARKS = 68
FEATURES = 256
HG_DEPTH = 4
MIN_MULTIPLE = 64          # stem /4, then four halvings inside the hourglass


class ConvBlock(nn.Module):
    """models.py:13-55 (parameters only)."""

    def __init__(self, in_planes, out_planes):
        super().__init__()
        self.in_planes, self.out_planes = in_planes, out_planes
        self.bn1 = nn.BatchNorm2d(in_planes)
        self.conv1 = nn.Conv2d(in_planes, out_planes // 2, 3, 1, 1, bias=False)
        self.bn2 = nn.BatchNorm2d(out_planes // 2)
        self.conv2 = nn.Conv2d(out_planes // 2, out_planes // 4, 3, 1, 1, bias=False)
        self.bn3 = nn.BatchNorm2d(out_planes // 4)
        self.conv3 = nn.Conv2d(out_planes // 4, out_planes // 4, 3, 1, 1, bias=False)
        if in_planes != out_planes:
            self.downsample = nn.Sequential(nn.BatchNorm2d(in_planes), nn.ReLU(True),
                                            nn.Conv2d(in_planes, out_planes, 1, 1, bias=False))
        else:
            self.downsample = None


class HourGlass(nn.Module):
    """models.py:98-142 (parameters only)."""

    def __init__(self, num_modules, depth, num_features):
        super().__init__()
        self.num_modules, self.depth, self.features = num_modules, depth, num_features
        self._generate_network(depth)

    def _generate_network(self, level):
        self.add_module("b1_" + str(level), ConvBlock(self.features, self.features))
        self.add_module("b2_" + str(level), ConvBlock(self.features, self.features))
        if level > 1:
            self._generate_network(level - 1)
        else:
            self.add_module("b2_plus_" + str(level), ConvBlock(self.features, self.features))
        self.add_module("b3_" + str(level), ConvBlock(self.features, self.features))


class FANParams(nn.Module):
    """models.py:145-172."""

    def __init__(self, num_modules=4):
        super().__init__()
        self.num_modules = num_modules
        self.conv1 = nn.Conv2d(3, 64, 7, 2, 3)
        self.bn1 = nn.BatchNorm2d(64)
        self.conv2 = ConvBlock(64, 128)
        self.conv3 = ConvBlock(128, 128)
        self.conv4 = ConvBlock(128, FEATURES)
        for i in range(num_modules):
            self.add_module("m" + str(i), HourGlass(1, HG_DEPTH, FEATURES))
            self.add_module("top_m_" + str(i), ConvBlock(FEATURES, FEATURES))
            self.add_module("conv_last" + str(i), nn.Conv2d(FEATURES, FEATURES, 1, 1, 0))
            self.add_module("bn_end" + str(i), nn.BatchNorm2d(FEATURES))
            self.add_module("l" + str(i), nn.Conv2d(FEATURES, NUM_LANDMARKS, 1, 1, 0))
            if i < num_modules - 1:
                self.add_module("bl" + str(i), nn.Conv2d(FEATURES, FEATURES, 1, 1, 0))
                self.add_module("al" + str(i), nn.Conv2d(NUM_LANDMARKS, FEATURES, 1, 1, 0))


def check_input(h: int, w: int):
    if h <= 0 or w <= 0 or h % MIN_MULTIPLE or w % MIN_MULTIPLE:
        raise ValueError(f"FAN: a {h}x{w} input; both sides must be positive multiples of {MIN_MULTIPLE} "
                         "(the stem quarters the map and the hourglass halves it four times)")


def conv_blocks(num_modules=4) -> int:
    """ConvBlocks per forward: 3 in the stem, 13 per hourglass and one top_m per stack."""
    return 3 + num_modules * (3 * HG_DEPTH + 1 + 1)
