"""GANimation's SplitGenerator (third_part/ganimation_replicate/model/model_utils.py:209-248, 419-482),
NHWC on libs2v.

Every layer is s2v_conv2d followed by the affine-free InstanceNorm2d pass (ops.instnorm, eps 1e-5, biased
variance) that also applies what follows the norm in the reference:
  * stem 7x7 (20 -> 64) and the two 4x4 stride-2 stages (64 -> 128 -> 256): conv, then IN + ReLU;
  * six ResnetBlocks ``x + IN(conv3x3(ReLU(IN(conv3x3(x)))))``: the first IN carries the ReLU, the second
    the residual (``res=``);
  * the two ConvTranspose2d(4, stride 2, padding 1) stages (256 -> 128 -> 64) run as their four output
    parity classes of 2x2 taps each (ConvW.make_polyphase), then IN + ReLU;
  * color_top (64 -> 3) and au_top (64 -> 1), both 7x7 without bias on the same features, are ONE conv of
    stacked weights [4, 64, 7, 7] writing the raw logits; tanh / sigmoid and the blend are s2v_gani_blend.

Every conv but the heads sits directly in front of an InstanceNorm2d(affine=False), which removes any
per-channel constant: the conv biases (all present in the state_dict) cancel exactly and are not applied.

Launches per forward (LAUNCHES): 1 + 2 + 12 convs, 2 x 4 parity classes, the head: 24 convs; 17 norm passes.
"""
from __future__ import annotations

import torch

from .. import ops
from ..models import ganimation_arch as arch
from ..ops import NHWC, ConvW

RELU = ops.ACT_RELU
HEAD_CS = 4                                # colour logits 0-2, mask logit 3: one float4 per pixel
CONVS = 1 + len(arch.DOWN) + 2 * len(arch.BLOCKS) + 4 * len(arch.UP) + 1
NORMS = 1 + len(arch.DOWN) + 2 * len(arch.BLOCKS) + len(arch.UP)
LAUNCHES = CONVS + NORMS


class GANimationEngine:
    def __init__(self, sd, device):
        dev = torch.device(device)
        self.device = dev

        def w(name):
            return sd[name + ".weight"].float()
        self.stem = ConvW(w("model.0"), None, dev, padding=3)
        self.down = [ConvW(w(f"model.{i}"), None, dev, stride=2, padding=1) for i, _, _ in arch.DOWN]
        self.blocks = [(ConvW(w(f"model.{i}.conv_block.0"), None, dev, padding=1),
                        ConvW(w(f"model.{i}.conv_block.3"), None, dev, padding=1)) for i in arch.BLOCKS]
        self.up = [ConvW(w(f"model.{i}"), None, dev, stride=2, padding=1, transposed=True).make_polyphase(dev)
                   for i, _, _ in arch.UP]
        self.head = ConvW(torch.cat([w("color_top.0"), w("au_top.0")]), None, dev, padding=3)

    @staticmethod
    def _norm(ctx, x: NHWC, *, act=ops.ACT_NONE, res: NHWC | None = None) -> NHWC:
        y = NHWC.empty(x.n, x.h, x.w, x.c, x.t.device)
        return ops.instnorm(ctx, x, y, act=act, res=res, eps=arch.IN_EPS)

    @staticmethod
    def _conv(ctx, x: NHWC, cw: ConvW) -> NHWC:
        oh, ow = cw.out_hw(x.h, x.w)
        y = NHWC.empty(x.n, oh, ow, cw.cout, x.t.device)
        return ops.conv2d(ctx, x, cw, y)

    def forward(self, ctx, x20: NHWC):
        """x20 [n, H, W, 20] fp32 (image in [-1, 1] | 17 constant action-unit channels; H, W multiples of 4)
        -> (head logits NHWC [n, H, W, 4], embed_features NHWC [n, H, W, 64])."""
        arch.check_input(x20.h, x20.w)             # ValueError before any launch
        if x20.c != arch.IMG_NC + arch.AUS_NC:
            raise ValueError(f"GANimation: the input has {x20.c} channels, not {arch.IMG_NC + arch.AUS_NC}")
        h = self._norm(ctx, self._conv(ctx, x20, self.stem), act=RELU)
        for cw in self.down:
            h = self._norm(ctx, self._conv(ctx, h, cw), act=RELU)
        for c1, c2 in self.blocks:
            t = self._norm(ctx, self._conv(ctx, h, c1), act=RELU)
            h = self._norm(ctx, self._conv(ctx, t, c2), res=h)
        for cw in self.up:
            h = self._norm(ctx, self._conv(ctx, h, cw), act=RELU)
        head = NHWC.empty(h.n, h.h, h.w, HEAD_CS, h.t.device)
        ops.conv2d(ctx, h, self.head, head)
        return head, h
