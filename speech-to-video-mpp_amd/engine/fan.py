"""FAN engine (third_part/face_detection/models.py:13-201), NHWC on libs2v.

FAN is pre-activation: every conv reads relu(bn(x)) while the raw x feeds the residual and the channel
concat, and s2v_conv2d's prologue has no shift, so the BN + ReLU passes are kernels of their own
(csrc/fan.hip), fused so that a tensor is read once for everything derived from it:

  * eval BatchNorm is scale = w / sqrt(var + 1e-5), shift = b - mean * scale;
  * conv1 + bn1 + relu and conv_last + bn_end + relu fold into conv epilogues;
  * a ConvBlock's three convs write their slices of ONE concat buffer (torch.cat disappears); bn2 / bn3
    + relu read those slices (s2v_bn_act_nhwc);
  * the block's ``out3 += residual`` is s2v_fan_merge, which also writes what the consumers of the sum
    need: relu(bn1(.)) of the next block, the hourglass's F.avg_pool2d(inp, 2, 2) and the pooled
    branch's relu(bn1(.)).  A block with a downsample adds the concat buffer in the 1x1 conv's residual
    epilogue instead;
  * the hourglass's ``up1 + F.interpolate(low3, 2, 'nearest')`` is one s2v_fan_merge (half-size b);
  * ``previous + bl(ll) + al(tmp_out)`` is the residual epilogue of the bl and al convs.

Launches per forward (LAUNCH_BUDGET; FAN-4 has 59 ConvBlocks): a ConvBlock is 3 convs + 2 BN passes +
its merge (6), or, with a downsample, + the downsample's BN pass with the 1x1 conv in place of the merge
(7); a stack outside its blocks is its input merge + 4 upsample merges + conv_last + l + bl + al (9, the
last stack 7); the stem outside its blocks is conv1, conv2's bn1 pass and the pool merge (3).
"""
from __future__ import annotations

import torch

from .. import ops
from ..models import fan_arch
from ..ops import NHWC, ConvW

RELU = ops.ACT_RELU
BN_EPS = 1e-5
HM_CS = fan_arch.NUM_LANDMARKS          # pixel pitch of the heatmaps (68 floats: 16-byte aligned rows)

# at most 7 launches per ConvBlock, 9 per stack outside its blocks, 3 for the stem
LAUNCH_BUDGET = 7 * fan_arch.conv_blocks(4) + 9 * 4 + 3


def bn_fold(sd, prefix, device):
    """Eval BatchNorm2d ``prefix`` -> (scale, shift) device tensors."""
    g, b, m, v = (sd[prefix + k].float() for k in ("weight", "bias", "running_mean", "running_var"))
    s = g / torch.sqrt(v + BN_EPS)
    return s.contiguous().to(device), (b - m * s).contiguous().to(device)


def bn_act(ctx, x: NHWC, bn, y: NHWC | None = None) -> NHWC:
    """relu(x * scale + shift) of a channel view into ``y`` (a new tensor by default)."""
    if y is None:
        y = NHWC.empty(x.n, x.h, x.w, x.c, x.t.device)
    assert (y.n, y.h, y.w, y.c) == (x.n, x.h, x.w, x.c) and bn[0].numel() == x.c
    ops.check(ctx.lib.s2v_bn_act_nhwc(x.t.data_ptr(), x.n * x.h * x.w, x.c, x.cs, x.coff, bn[0].data_ptr(),
                                      bn[1].data_ptr(), y.t.data_ptr(), y.cs, y.coff, ctx.stream), "s2v_bn_act_nhwc")
    return y


def merge(ctx, a: NHWC, b: NHWC | None = None, *, want_s=True, bn_a=None, pool=False, bn_b=None):
    """s = a + b (b: None, same size, or half size read with nearest x2) -> (s, relu(bn_a(s)), p,
    relu(bn_b(p))) with p the 2x2 mean of s; outputs not asked for are None."""
    dev = a.t.device
    half = b is not None and (b.h, b.w) != (a.h, a.w)
    assert b is None or ((b.n, b.c) == (a.n, a.c) and (b.h, b.w) == ((a.h // 2, a.w // 2) if half else (a.h, a.w)))
    s = NHWC.empty(a.n, a.h, a.w, a.c, dev) if want_s else None
    sa = NHWC.empty(a.n, a.h, a.w, a.c, dev) if bn_a is not None else None
    p = NHWC.empty(a.n, a.h // 2, a.w // 2, a.c, dev) if pool else None
    pa = NHWC.empty(a.n, a.h // 2, a.w // 2, a.c, dev) if bn_b is not None else None

    def pc(v):
        return (v.ptr, v.cs) if v is not None else (None, 0)

    def pt(t):
        return None if t is None else t.data_ptr()
    bn_a = bn_a or (None, None)
    bn_b = bn_b or (None, None)
    ops.check(ctx.lib.s2v_fan_merge(a.ptr, a.cs, *pc(b), int(half), a.n, a.h, a.w, a.c, *pc(s), *pc(sa), pt(bn_a[0]),
                                    pt(bn_a[1]), *pc(p), *pc(pa), pt(bn_b[0]), pt(bn_b[1]), ctx.stream),
              "s2v_fan_merge")
    return s, sa, p, pa


class _Block:
    """Folded weights of one ConvBlock."""

    def __init__(self, sd, prefix, dev):
        w1 = sd[prefix + "conv1.weight"]
        self.cin, self.cout = int(w1.shape[1]), 2 * int(w1.shape[0])
        self.bn1, self.bn2, self.bn3 = (bn_fold(sd, f"{prefix}bn{i}.", dev) for i in (1, 2, 3))
        self.c1, self.c2, self.c3 = (ConvW(sd[f"{prefix}conv{i}.weight"].float(), None, dev, padding=1)
                                     for i in (1, 2, 3))
        self.ds = None
        if prefix + "downsample.2.weight" in sd:
            self.ds = (bn_fold(sd, prefix + "downsample.0.", dev),
                       ConvW(sd[prefix + "downsample.2.weight"].float(), None, dev))

    def concat(self, ctx, x: NHWC, a1: NHWC) -> NHWC:
        """torch.cat((out1, out2, out3), 1) from a1 = relu(bn1(x)): 3 convs + 2 BN passes."""
        c = self.cout
        cat = NHWC.empty(x.n, x.h, x.w, c, x.t.device)
        o1, o2, o3 = cat.slice(0, c // 2), cat.slice(c // 2, c // 4), cat.slice(3 * c // 4, c // 4)
        ops.conv2d(ctx, a1, self.c1, o1)
        ops.conv2d(ctx, bn_act(ctx, o1, self.bn2), self.c2, o2)
        ops.conv2d(ctx, bn_act(ctx, o2, self.bn3), self.c3, o3)
        return cat

    def __call__(self, ctx, x: NHWC, a1: NHWC, **outs):
        """The block on raw x with a1 = relu(bn1(x)) -> merge()'s tuple of the block output (``outs``:
        merge's keywords).  A downsample block returns (out, None, None, None)."""
        cat = self.concat(ctx, x, a1)
        if self.ds is None:
            return merge(ctx, cat, x, **outs)
        assert not outs, "a downsample block only produces its sum"
        out = NHWC.empty(x.n, x.h, x.w, self.cout, x.t.device)
        ops.conv2d(ctx, bn_act(ctx, x, self.ds[0]), self.ds[1], out, res=cat)
        return out, None, None, None


class FANEngine:
    def __init__(self, sd, device):
        dev = torch.device(device)
        self.device = dev
        self.num_modules = 1 + max(int(k[len("conv_last"):].split(".")[0]) for k in sd if k.startswith("conv_last"))
        bn1 = tuple(sd["bn1." + k] for k in ("weight", "bias", "running_mean", "running_var"))
        self.stem = ConvW(ops.pad_cin(sd["conv1.weight"].float(), 4), sd["conv1.bias"], dev, stride=2, padding=3,
                          bn=bn1, bn_eps=BN_EPS)
        self.conv2, self.conv3, self.conv4 = (_Block(sd, f"conv{i}.", dev) for i in (2, 3, 4))
        self.stacks = []
        for i in range(self.num_modules):
            hg = {}
            for lv in range(fan_arch.HG_DEPTH, 0, -1):
                for b in ("b1_", "b2_", "b3_") + (("b2_plus_",) if lv == 1 else ()):
                    hg[b + str(lv)] = _Block(sd, f"m{i}.{b}{lv}.", dev)
            bn_end = tuple(sd[f"bn_end{i}." + k] for k in ("weight", "bias", "running_mean", "running_var"))
            st = dict(hg=hg, top=_Block(sd, f"top_m_{i}.", dev),
                      last=ConvW(sd[f"conv_last{i}.weight"].float(), sd[f"conv_last{i}.bias"], dev, bn=bn_end,
                                 bn_eps=BN_EPS),
                      l=ConvW(sd[f"l{i}.weight"].float(), sd[f"l{i}.bias"], dev))
            if i < self.num_modules - 1:
                st["bl"] = ConvW(sd[f"bl{i}.weight"].float(), sd[f"bl{i}.bias"], dev)
                st["al"] = ConvW(sd[f"al{i}.weight"].float(), sd[f"al{i}.bias"], dev)
            self.stacks.append(st)

    def _hourglass(self, ctx, hg, level, inp, a_b1, low, a_b2, out_bn):
        """HourGlass._forward(level, inp) with a_b1 = relu(b1.bn1(inp)), low = avg_pool(inp), a_b2 =
        relu(b2.bn1(low)) -> (up1 + up2, relu(out_bn(up1 + up2)))."""
        up1 = hg[f"b1_{level}"](ctx, inp, a_b1)[0]
        b2 = hg[f"b2_{level}"]
        if level > 1:
            nb1, nb2 = hg[f"b1_{level - 1}"], hg[f"b2_{level - 1}"]
            low1, a1, p, pa = b2(ctx, low, a_b2, bn_a=nb1.bn1, pool=True, bn_b=nb2.bn1)
            low2, a3 = self._hourglass(ctx, hg, level - 1, low1, a1, p, pa, hg[f"b3_{level}"].bn1)
        else:
            plus = hg["b2_plus_1"]
            low1, a1, _, _ = b2(ctx, low, a_b2, bn_a=plus.bn1)
            low2, a3, _, _ = plus(ctx, low1, a1, bn_a=hg["b3_1"].bn1)
        low3 = hg[f"b3_{level}"](ctx, low2, a3)[0]
        s, sa, _, _ = merge(ctx, up1, low3, bn_a=out_bn)
        return s, sa

    def forward(self, ctx, x4: NHWC):
        """x4 [n, H, W, 4] fp32 (RGB / 255, channel 3 zero; H, W multiples of 64) -> the heatmaps of all
        stacks, NHWC [n, H/4, W/4, HM_CS] each."""
        fan_arch.check_input(x4.h, x4.w)
        dev = x4.t.device
        n, h, w = x4.n, x4.h // 2, x4.w // 2
        x = NHWC.empty(n, h, w, 64, dev)
        ops.conv2d(ctx, x4, self.stem, x, act=RELU)
        out = self.conv2(ctx, x, bn_act(ctx, x, self.conv2.bn1))[0]
        _, _, p, pa = merge(ctx, out, None, want_s=False, pool=True, bn_b=self.conv3.bn1)
        x, a1, _, _ = self.conv3(ctx, p, pa, bn_a=self.conv4.bn1)
        previous = self.conv4(ctx, x, a1)[0]
        outputs = []
        for i, st in enumerate(self.stacks):
            hg = st["hg"]
            top = fan_arch.HG_DEPTH
            _, a_b1, low, a_b2 = merge(ctx, previous, None, want_s=False, bn_a=hg[f"b1_{top}"].bn1, pool=True,
                                       bn_b=hg[f"b2_{top}"].bn1)
            s, sa = self._hourglass(ctx, hg, top, previous, a_b1, low, a_b2, st["top"].bn1)
            ll = st["top"](ctx, s, sa)[0]
            feat = NHWC.empty(n, ll.h, ll.w, fan_arch.FEATURES, dev)
            ops.conv2d(ctx, ll, st["last"], feat, act=RELU)
            hm = NHWC.empty(n, ll.h, ll.w, HM_CS, dev)
            ops.conv2d(ctx, feat, st["l"], hm.slice(0, fan_arch.NUM_LANDMARKS))
            outputs.append(hm)
            if "bl" in st:
                # previous + bl(ll) + al(tmp_out): two residual epilogues, in the reference's order
                t = NHWC.empty(n, ll.h, ll.w, fan_arch.FEATURES, dev)
                ops.conv2d(ctx, feat, st["bl"], t, res=previous)
                previous = NHWC.empty(n, ll.h, ll.w, fan_arch.FEATURES, dev)
                ops.conv2d(ctx, hm.slice(0, fan_arch.NUM_LANDMARKS), st["al"], previous, res=t)
        return outputs

    @staticmethod
    def to_nchw(maps):
        """NHWC heatmaps -> the reference's list of [n, 68, h, w] tensors."""
        return [m.t[..., : fan_arch.NUM_LANDMARKS].permute(0, 3, 1, 2).contiguous() for m in maps]
