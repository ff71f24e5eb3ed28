"""GANimation upper-face editing (--up_face) and the --without_rl1 composite on the device: the names of
third_part/ganimation_replicate/model/ganimation.py and of inference.py:250-253, :269-288.

Per batch the reference resizes the uint8 originals to 128 x 128 in [-1, 1], runs SplitGenerator on them with
the expression's 17 action units, blends ``fake = a * src + (1 - a) * color``, resizes fake / 2 + 0.5 back to
the prediction's size and, under --without_rl1, keeps the prediction where the network's input was zero (the
masked lower half, and any zero pixel above it) and the edited original elsewhere.  Here that is

    s2v_gani_input  ->  engine/ganimation.py (24 convs, 17 norm passes)  ->  s2v_gani_blend  ->  s2v_gani_compose

with no host step in between: the stage is captured into the pipeline's graphs like the networks around it.
The reference runs the generator whenever --up_face names an expression and then drops its output unless
--without_rl1 is given; the pipeline skips the forward in that case (the frames are the same).
There is no CPU path.
"""
from __future__ import annotations

import os

import torch

from . import ops, post
from ._lib import check
from .models import ganimation_arch
from .ops import NHWC

# futils/inference_utils.py:53-57; AU01, 02, 04, 05, 06, 07, 09, 10, 12, 14, 15, 17, 20, 23, 25, 26, 45
exp_aus_dict = {
    "sad": torch.zeros(1, ganimation_arch.AUS_NC),
    "angry": torch.zeros(1, ganimation_arch.AUS_NC).index_fill_(1, torch.tensor([2]), 0.3),
    "surprise": torch.zeros(1, ganimation_arch.AUS_NC).index_fill_(1, torch.tensor([3]), 0.2),
}
FINAL_SIZE = 128                  # the generator's working size (inference.py:277)
CKPT_NAME = "30_net_gen.pth"      # base_model.py:125


def check_up_face(name):
    """The expression names inference.py:269 knows; the reference fails on any other with a NameError at
    the first batch, here it is a ValueError before any launch."""
    if name not in exp_aus_dict:
        raise ValueError(f"up_face {name!r}: one of {sorted(exp_aus_dict)} (or 'original' for no edit)")
    return name


def _u8_hwc(t: torch.Tensor, what: str):
    if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.uint8 and t.dim() == 4 and
            t.shape[3] == 3 and t.stride(3) == 1 and t.stride(2) == 3):
        raise RuntimeError(f"{what}: expected uint8 [N,H,W,3] HIP device images (rows may be views of a larger "
                           "frame), there is no CPU fallback")
    return post._hwc(t)


def gani_input(ctx, orig_u8: torch.Tensor, aus: torch.Tensor, size=(FINAL_SIZE, FINAL_SIZE)) -> NHWC:
    """uint8 originals [N,P,Q,3] and action units [N,17] -> the generator input NHWC [N,H,W,20] (s2v_gani_input)."""
    n, h, w, _, xrs, xis = _u8_hwc(orig_u8, "gani_input")
    ops._require_cuda(aus, "gani_input aus")
    if tuple(aus.shape) != (n, ganimation_arch.AUS_NC) or not aus.is_contiguous():
        raise ValueError(f"gani_input: aus {tuple(aus.shape)} must be contiguous [{n}, {ganimation_arch.AUS_NC}]")
    y = NHWC.empty(n, size[0], size[1], 3 + ganimation_arch.AUS_NC, orig_u8.device)
    check(ctx.lib.s2v_gani_input(orig_u8.data_ptr(), n, h, w, xrs, xis, aus.data_ptr(), y.ptr, size[0], size[1],
                                 ctx.stream), "s2v_gani_input")
    return y


def gani_compose(ctx, pred: torch.Tensor, orig_u8: torch.Tensor, fake: torch.Tensor | None, out: torch.Tensor):
    """inference.py:274-288 (s2v_gani_compose): pred fp32 [N,3,P,Q] and the uint8 originals [N,P,Q,3] with the
    edited faces ``fake`` [N,3,h,w] (None: the originals themselves, up_face 'original') -> ``out`` [N,3,P,Q],
    float32 (the blended frames) or uint8 (their ``* 255`` truncation)."""
    ops._require_cuda(pred, "gani_compose pred")
    n, c, ph, pw = pred.shape
    on, oh, ow, _, ors, ois = _u8_hwc(orig_u8, "gani_compose")
    if c != 3 or (on, oh, ow) != (n, ph, pw) or not pred.is_contiguous():
        raise ValueError(f"gani_compose: pred {tuple(pred.shape)} (contiguous [N,3,P,Q]) and originals "
                         f"{tuple(orig_u8.shape)} do not match")
    fh = fw = 0
    if fake is not None:
        ops._require_cuda(fake, "gani_compose fake")
        if fake.dim() != 4 or fake.shape[:2] != (n, 3) or not fake.is_contiguous():
            raise ValueError(f"gani_compose: fake_img {tuple(fake.shape)} must be contiguous [{n},3,h,w]")
        fh, fw = fake.shape[2:]
    if (out.dtype not in (torch.uint8, torch.float32) or tuple(out.shape) != (n, 3, ph, pw) or not out.is_cuda or
            not out.is_contiguous()):
        raise ValueError(f"gani_compose: out {tuple(out.shape)} {out.dtype} must be a contiguous device "
                         f"[{n},3,{ph},{pw}] of uint8 or float32")
    check(ctx.lib.s2v_gani_compose(pred.data_ptr(), orig_u8.data_ptr(), ors, ois,
                                   None if fake is None else fake.data_ptr(), fh, fw, n, ph, pw, out.data_ptr(),
                                   int(out.dtype == torch.uint8), ctx.stream), "s2v_gani_compose")
    return out


class GANimationModel:
    """model/ganimation.py:6-53 in test mode: ``initialize()``, ``setup()``, ``feed_batch({'src_img',
    'tar_aus'})``, ``forward()`` and the attributes ``color_mask``, ``aus_mask``, ``fake_img`` (NCHW device
    tensors).  ``embed`` (the reference's third generator output) is converted to NCHW only when read.
    ``edit`` is the pipeline's entry: uint8 originals in, ``fake_img`` out, nothing on the host."""

    exp_aus_dict = exp_aus_dict

    def __init__(self):
        self.name = "GANimation"
        self.is_train = False
        self.models_name = []
        self.net_gen = None
        self.device = "cuda"
        self.final_size = FINAL_SIZE
        self.color_mask = self.aus_mask = self.fake_img = None
        self._embed = None

    def initialize(self, ckpt_path: str | None = None, net_gen=None, device="cuda"):
        """``net_gen``: a models.SplitGenerator holding its weights; else the checkpoint ``ckpt_path``
        (default checkpoints/30_net_gen.pth, base_model.py:125), which must exist: nothing is downloaded."""
        from . import models
        if net_gen is None:
            path = ckpt_path or os.path.join("checkpoints", CKPT_NAME)
            if not os.path.isfile(path):
                raise FileNotFoundError(f"GANimation: no generator checkpoint at {path!r}")
            net_gen = models.load_ganimation(path)
        self.net_gen = net_gen
        self.models_name = ["gen"]
        self.device = torch.device(device)
        return self

    def setup(self):
        self.net_gen.eval()
        return self

    def feed_batch(self, batch):
        self.src_img = batch["src_img"].to(self.device)
        self.tar_aus = batch["tar_aus"].float().to(self.device)

    def _run(self, x20: NHWC, lane: int):
        (head, embed), ctx = self.net_gen.forward_nhwc(x20, lane)
        self.color_mask, self.aus_mask, self.fake_img = self.net_gen.blend(ctx, head, x20)
        self._embed = (ctx, embed)
        return self.fake_img

    @torch.no_grad()
    def forward(self):
        src, aus = self.src_img, self.tar_aus
        b, c, h, w = src.shape
        if c != 3 or tuple(aus.shape) != (b, ganimation_arch.AUS_NC):
            raise RuntimeError(f"GANimation: src_img {tuple(src.shape)} / tar_aus {tuple(aus.shape)}: expected "
                               "[B,3,H,W] and [B,17]")
        ganimation_arch.check_input(h, w)
        ctx = self.net_gen._engine(src.device)[1]
        x20 = NHWC.empty(b, h, w, 3 + ganimation_arch.AUS_NC, src.device)
        x20.t[..., 3:] = aus[:, None, None, :]
        ops.nchw_to_nhwc(ctx, src.float(), x20.slice(0, 3))
        self._run(x20, 0)

    @torch.no_grad()
    def edit(self, orig_u8: torch.Tensor, aus: torch.Tensor, lane: int = 0) -> torch.Tensor:
        """inference.py:277-280 on uint8 originals [B,P,P,3] with action units [B,17] (device): fake_img
        [B,3,128,128] in [-1, 1]."""
        ctx = self.net_gen._engine(orig_u8.device, lane)[1]
        return self._run(gani_input(ctx, orig_u8, aus, (self.final_size, self.final_size)), lane)

    @property
    def embed(self):
        """embed_features [B,64,H,W] of the last forward."""
        if self._embed is None:
            return None
        ctx, e = self._embed
        return ops.nhwc_to_nchw(ctx, e, torch.empty((e.n, e.c, e.h, e.w), device=e.t.device))
