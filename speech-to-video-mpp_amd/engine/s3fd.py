"""S3FD engine (third_part/face_detection/detection/sfd/net_s3fd.py:70-129), NHWC on libs2v.

Every conv is one s2v_conv2d launch with its bias and ReLU in the epilogue:
  * conv1_1 reads the 4-channel NHWC input (channel 3 zero, weights zero-padded to 4 input channels:
    the exact-fp32 4-channel path); the five F.max_pool2d(h, 2, 2) are s2v_maxpool2d_nhwc (2, 2, 0);
  * fc6 is a 3x3 conv with padding 3 (its map is 4 larger than its input), fc7 / conv6_1 / conv7_1
    are 1x1, conv6_2 / conv7_2 have stride 2;
  * conv3_3 / conv4_3 / conv5_3 are L2-normalised (s2v_l2norm_nhwc) into separate buffers that only the
    heads read; the pooled trunk continues from the un-normalised feature;
  * the class and box heads of a level are ONE 3x3 conv with concatenated weights writing
    [conf (4 on level 0, else 2) | loc (4)] into a map of pixel pitch HEAD_CS; s2v_s3fd_decode reads
    that layout (level-0 max-out, softmax, threshold, prior decode).
"""
from __future__ import annotations

import torch

from .. import ops
from ..models import s3fd_arch
from ..ops import NHWC, ConvW

RELU = ops.ACT_RELU


class S3FDEngine:
    HEAD_CS = 8

    def __init__(self, sd, device):
        dev = torch.device(device)
        self.device = dev
        self.trunk = []
        for name, cin, _, _, s, p in s3fd_arch.TRUNK:
            w = sd[name + ".weight"].float()
            if cin == 3:
                w = ops.pad_cin(w, 4)
            self.trunk.append((name, ConvW(w, sd[name + ".bias"], dev, stride=s, padding=p)))
        self.norms = {name[: -len("_norm")]: sd[name + ".weight"].float().contiguous().to(dev)
                      for name, _, _ in s3fd_arch.L2NORMS}
        self.heads = []
        for prefix, src, _, nconf in s3fd_arch.LEVELS:
            w = torch.cat([sd[f"{prefix}_mbox_conf.weight"], sd[f"{prefix}_mbox_loc.weight"]])
            b = torch.cat([sd[f"{prefix}_mbox_conf.bias"], sd[f"{prefix}_mbox_loc.bias"]])
            pad = self.HEAD_CS - w.shape[0]            # zero output channels up to the common pitch
            if pad:
                w = torch.cat([w, torch.zeros((pad,) + tuple(w.shape[1:]), dtype=w.dtype)])
                b = torch.cat([b, torch.zeros(pad, dtype=b.dtype)])
            self.heads.append((src, nconf, ConvW(w, b, dev, padding=1)))

    def _pool(self, ctx, x: NHWC) -> NHWC:
        oh, ow = x.h // 2, x.w // 2
        y = NHWC.empty(x.n, oh, ow, x.c, x.t.device)
        ops.check(ctx.lib.s2v_maxpool2d_nhwc(x.ptr, x.n, x.h, x.w, x.c, 2, 2, 0, y.ptr, oh, ow, ctx.stream),
                  "s2v_maxpool2d_nhwc")
        return y

    def _l2norm(self, ctx, x: NHWC, weight: torch.Tensor) -> NHWC:
        y = NHWC.empty(x.n, x.h, x.w, x.c, x.t.device)
        ops.check(ctx.lib.s2v_l2norm_nhwc(x.ptr, x.n * x.h * x.w, x.c, x.cs, weight.data_ptr(),
                                          s3fd_arch.L2NORM_EPS, y.ptr, y.cs, ctx.stream), "s2v_l2norm_nhwc")
        return y

    def sources(self, ctx, x4: NHWC):
        """x4 [n,H,W,4] (pixels minus the means, channel 3 zero) -> {trunk name: detection source}
        (conv3_3 / conv4_3 / conv5_3 L2-normalised)."""
        s3fd_arch.level_sizes(x4.h, x4.w)              # ValueError before any launch
        wanted = {src for src, _, _ in self.heads}
        out = {}
        h = x4
        for name, cw in self.trunk:
            oh, ow = cw.out_hw(h.h, h.w)
            y = NHWC.empty(h.n, oh, ow, cw.cout, h.t.device)
            ops.conv2d(ctx, h, cw, y, act=RELU)
            h = y
            if name in wanted:
                out[name] = self._l2norm(ctx, h, self.norms[name]) if name in self.norms else h
            if name in s3fd_arch.POOL_AFTER:
                h = self._pool(ctx, h)
        return out

    def forward_maps(self, ctx, x4: NHWC):
        """-> the six fused head maps [n, h_l, w_l, HEAD_CS]; channels past a level's conf + loc are
        zero and never read."""
        feats = self.sources(ctx, x4)
        maps = []
        for src, nconf, cw in self.heads:
            f = feats[src]
            m = NHWC.empty(f.n, f.h, f.w, self.HEAD_CS, f.t.device)
            ops.conv2d(ctx, f, cw, m)
            maps.append(m)
        return maps

    @staticmethod
    def split_heads(maps):
        """Head maps -> the reference's list [cls1, reg1, .., cls6, reg6] in NCHW, level-0 conf max-outed
        to (max(c0, c1, c2), c3) (net_s3fd.py:124-129)."""
        outs = []
        for lv, m in enumerate(maps):
            t = m.t
            if lv == 0:
                conf = torch.cat([t[..., 0:3].amax(dim=3, keepdim=True), t[..., 3:4]], 3)
                loc = t[..., 4:8]
            else:
                conf, loc = t[..., 0:2], t[..., 2:6]
            outs += [conf.permute(0, 3, 1, 2).contiguous(), loc.permute(0, 3, 1, 2).contiguous()]
        return outs
