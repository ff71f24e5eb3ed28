"""Inputs shared by the GANimation tests and tests/golden/make_ganimation_golden.py (everything is regenerated
from its key, so the fixture holds only recorded results), and restatements of the three kernels of
csrc/gani.hip and of inference.py:277-288 in torch on the CPU (fp32 as the reference computes them; fp64 where
a test wants the exact value)."""
import numpy as np
import torch
import torch.nn.functional as F

from s2v_amd import synth

AUS_NC = 17
# name -> (batch, height, width) of the generator's input
CASES = {"b2_32": (2, 32, 32), "b1_44x36": (1, 44, 36), "b2_128": (2, 128, 128)}
COMPOSE_CASE, COMPOSE_P = "b2_128", 384          # lines 277-286 are probed on this case at P = 384
PROBES = 2048


def forward_eps(ref_max: float) -> float:
    """The project's forward bar: 1e-3 of the reference's largest magnitude, at least 1e-3."""
    return 1e-3 * max(1.0, float(ref_max))


def state_dict():
    from s2v_amd.models.ganimation_arch import SplitGeneratorParams
    return synth.synth_torch_state_dict(SplitGeneratorParams(), **synth.GANIMATION_SYNTH)


def net_inputs(case):
    """(src_img [B,3,H,W] in [-1, 1), tar_aus [B,17] in [0, 1))."""
    b, h, w = CASES[case]
    return (torch.from_numpy(synth.hash_array(f"ganimation.{case}.img", (b, 3, h, w), -1.0, 1.0)),
            torch.from_numpy(synth.hash_array(f"ganimation.{case}.aus", (b, AUS_NC), 0.0, 1.0)))


def image_u8(key, n, h, w):
    """uint8 [n, h, w, 3] noise."""
    return np.floor(synth.hash_array(f"ganimation.{key}", (n, h, w, 3), 0.0, 256.0)).clip(0, 255).astype(np.uint8)


def originals(key, n, h, w):
    """uint8 originals for the composite: noise without zeros, then single-channel zeros sprinkled over the
    top half (about one element in 16; they switch the mask per channel) while the bottom half stays
    non-zero (there the mask comes from the row alone)."""
    u = np.maximum(image_u8(key, n, h, w), 1)
    z = synth.hash_array(f"ganimation.{key}.zero", (n, h, w, 3), 0.0, 1.0) < 1.0 / 16
    z[:, h // 2:] = False
    u[z] = 0
    return u


def pred_values(key, n, h, w):
    """A prediction [n,3,h,w] with values on both sides of [0, 1] (ENet's output is unclamped)."""
    return torch.from_numpy(synth.hash_array(f"ganimation.{key}.pred", (n, 3, h, w), -0.25, 1.25))


def compose_inputs():
    """(pred [B,3,P,P], uint8 originals [B,P,P,3]) of the fixture's 277-286 probes."""
    b = CASES[COMPOSE_CASE][0]
    return pred_values("compose", b, COMPOSE_P, COMPOSE_P), originals("compose", b, COMPOSE_P, COMPOSE_P)


def probe(t, key):
    """synth.probe_indices samples of a tensor / array, flat."""
    a = t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)
    return a.reshape(-1)[synth.probe_indices(a.size, PROBES, key)]


# ----------------------------------------------------------------------------- restatements
def src128(orig_u8, size=(128, 128)):
    """inference.py:262, :277: F.interpolate(img_original * 2 - 1, size, 'bilinear') of the uint8 HWC originals."""
    img = torch.as_tensor(orig_u8).permute(0, 3, 1, 2).float() / 255.
    return F.interpolate(img * 2 - 1, size=tuple(size), mode="bilinear")


def input_ref(orig_u8, aus, size=(128, 128)):
    """s2v_gani_input: NHWC [B, h, w, 20] = cat(src128, aus broadcast) (model_utils.py:476-478)."""
    img = src128(orig_u8, size)
    au = torch.as_tensor(aus).float()[:, :, None, None].expand(-1, -1, *img.shape[2:])
    return torch.cat([img, au], 1).permute(0, 2, 3, 1).contiguous()


def blend_ref(head, src, dtype=torch.float64):
    """s2v_gani_blend: head logits [B,4,H,W] (colour 0-2, mask 3) and src [B,3,H,W] -> (color_mask, aus_mask,
    fake_img) as color_top / au_top / GANimationModel.forward compute them."""
    head, src = torch.as_tensor(head).to(dtype), torch.as_tensor(src).to(dtype)
    color, a = torch.tanh(head[:, :3]), torch.sigmoid(head[:, 3:4])
    return color, a, a * src + (1 - a) * color


def compose_ref(pred, orig_u8, fake, dtype=torch.float32):
    """inference.py:262-288 after the network: -> (blended frames [B,3,P,Q] float, their uint8 frames as
    ``(pred * 255.).astype(np.uint8)`` gives them).  fake None: up_face == 'original'."""
    orig_u8 = np.asarray(orig_u8)
    p, q = orig_u8.shape[1:3]
    img_original = torch.from_numpy(orig_u8.transpose(0, 3, 1, 2).copy()).to(dtype) / 255.
    img_masked = orig_u8.copy()
    img_masked[:, p // 2:] = 0                                             # :397
    incomplete = torch.from_numpy((img_masked / 255.).transpose(0, 3, 1, 2).copy()).to(dtype)
    pred = torch.clamp(torch.as_tensor(pred).to(dtype), 0, 1)              # :267
    if fake is None:
        cur = img_original                                                 # :275
    else:
        cur = F.interpolate(torch.as_tensor(fake).to(dtype) / 2. + 0.5, size=(p, q), mode="bilinear")   # :281
    mask = torch.where(incomplete == 0, torch.ones_like(incomplete), torch.zeros_like(incomplete))      # :285
    out = pred * mask + cur * (1 - mask)                                   # :286
    return out, (out.numpy() * 255.).astype(np.uint8)                      # :288, :294
