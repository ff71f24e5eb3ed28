"""The inference.py contract on a short clip (BASELINE configs[0]: examples/face/1.mp4 +
examples/audio/1.wav, 8 frames, plumbing).

    python -m s2v_amd.inference --face examples/face/1.mp4 --audio examples/audio/1.wav \
        --max_frames 8 --outfile results/out.npz

Steps (reference file:line in brackets):
  * audio: stdlib ``wave`` PCM -> float32, channels averaged, resampled to 16 kHz
    (audio.load_wav = librosa.load(path, sr=16000), futils/audio.py:10-11), or with --audio_load device the same
    three steps in one kernel on the file's sample bytes (s2v_amd.audio.load_audio) -> mel on the device ->
    16-column windows at 80 / fps columns per frame [inference.py:204-216];
  * video: --face NAME.avi is a Motion-JPEG AVI (``ffmpeg -i in.mp4 -c:v mjpeg -q:v 2 out.avi``): s2v_amd.mjpeg
    reads the container and decodes the frames on the device (JpegDecoder, batches of --LNet_batch_size), fps from
    the header; --face NAME.jpg is the reference's static mode [inference.py:58-64, :371]: the one frame for every
    mel window, at --fps.  There is no MP4 decoder: of an MP4 the header gives frame size, fps and frame count and
    the frames are synthetic uint8 BGR frames of that size (SURVEY.md §8d allows this); an .npy [N,H,W,3] uint8
    array is taken as it is;
  * frames truncated to the number of mel windows [inference.py:219-221];
  * the face box: by default the centred square of --box_frac of the short side; with --face_det the
    reference's face_detect [inference.py:357, futils/inference_utils.py:110-148] on the device
    (s2v_amd.face_detection: S3FD on every frame in batches of --face_det_batch_size, --pads, clamping,
    the 5-frame smoothing unless --nosmooth), giving one box per frame;
  * 3DMM coefficients: with --checkpoints holding face3d's epoch_20.pth, the built extractor
    (s2v_amd.face3d.Face3DExtractor: align_img + ReconNetWrapper('resnet50'), facing.py:100-130)
    regresses them from the frames with the box-derived 5 landmarks; otherwise they are synthetic;
    with --landmarks the 68 FAN landmarks of every frame (facing.py:89-97: KeypointExtractor over S3FD +
    FAN, weights from <checkpoints>/s3fd.pth and 2DFAN4.pth or the synthetic presets) drive align_img
    instead of the no-landmark path; with --geometry device the arithmetic between these networks (the landmarks'
    map back to the frame, align_img's parameters and their validation, the DNet coefficient windows) runs on
    the device as well, with the host routes' results;
  * DNet stabilisation of the box crop (trans_image: 256x256, [-1, 1], facing.py:177-191) with the
    coefficient windows, then ENet(LNet) on [masked crop, reference] batches of LNet_batch_size,
    clamp(0, 1) * 255 [inference.py:259-267, :393-399] (s2v_amd.pipeline.LipSyncPipeline);
  * --ref_enhance: Step 5, ``ref_enhancer.process(img, img, face_enhance=False)`` with
    FaceEnhancement(in_size 512, use_sr False) on every stabilised reference before ENet
    [inference.py:224-238] (needs real RetinaFace / ParseNet weights: synthetic ones detect no face,
    and the reference raises on a frame without one);
  * --stitch: datagen's reference construction [inference.py:348-367; futils/alignment_stit.py] on every
    stabilised reference before ENet (s2v_amd.stitch.Stitcher): the 68 FAN landmarks of the stabilised frame ->
    the rotated square around eyes and mouth -> Pillow QUAD crop -> inverse perspective paste over the original
    crop, then the two cv2 resizes into the face box and back.  Synthetic FAN weights give points that are no
    face: a frame whose quad is not finite or needs the reference's shrink branch raises, as the reference does;
  * --up_face sad|angry|surprise with --without_rl1: GANimation's upper-face edit [inference.py:250-253, :269-286]
    (s2v_amd.ganimation): the 384x384 original crops, resized to 128x128, go through SplitGenerator with the
    expression's action units; the edited faces, resized back, replace the prediction wherever the network's
    masked input was not zero (the upper half).  --without_rl1 alone composites the unedited crops.  Weights from
    <checkpoints>/30_net_gen.pth, or the synthetic preset without it.  --up_face without --without_rl1 changes
    nothing (the reference computes the edit and drops it; here it is not computed);
  * each 384x384 prediction resized into the box and pasted into its frame [inference.py:287-291];
  * --enhance: FaceEnhancement (SR x2, RetinaFace, GPEN-2048, parse-mask paste) on each pasted frame
    against the 2x frame [inference.py:228-231, :317-328]; needs real checkpoints (synthetic
    RetinaFace weights detect no faces, and the reference raises on a frame without one).
  * --outfile NAME.avi: the frames (the --enhance output when there is one) as a Motion-JPEG AVI with the
    audio of --audio, the counterpart of cv2.VideoWriter + the ffmpeg mux [inference.py:246-249, :325-336]:
    baseline JPEG on the device at --jpeg_quality (s2v_amd.mjpeg, in batches of --LNet_batch_size), PCM at
    the file's own rate and channel count cut to the clip.  Any other extension: the arrays as an .npz.
Weights come from --checkpoints (LNet.pth / ENet.pth / DNet.pt as models.load_network /
load_DNet read them) or, when absent, from the portable synthetic generator (s2v_amd.synth).
"""
from __future__ import annotations

import argparse
import json
import math
import os
import struct
import sys
import time
import wave

import numpy as np
import torch


# ----------------------------------------------------------------------------- audio
def _pcm_to_float(raw: bytes, width: int) -> np.ndarray:
    if width == 1:
        return (np.frombuffer(raw, np.uint8).astype(np.float32) - 128.0) / 128.0
    if width == 2:
        return np.frombuffer(raw, "<i2").astype(np.float32) / 32768.0
    if width == 3:
        b = np.frombuffer(raw, np.uint8).reshape(-1, 3).astype(np.int32)
        v = b[:, 0] | (b[:, 1] << 8) | (b[:, 2] << 16)
        return (np.where(v >= 1 << 23, v - (1 << 24), v)).astype(np.float32) / float(1 << 23)
    if width == 4:
        return np.frombuffer(raw, "<i4").astype(np.float32) / float(1 << 31)
    raise ValueError(f"unsupported PCM sample width {width}")


def resample(x: np.ndarray, sr_in: int, sr_out: int, num_zeros: int = 64, rolloff: float = 0.9475937167399596,
             beta: float = 14.769656459379492) -> np.ndarray:
    """Band-limited (Kaiser-windowed sinc) resampling with librosa 0.9's default 'kaiser_best'
    parameters (resampy: 64 zero crossings, rolloff 0.9476, Kaiser beta 14.77).  resampy's tabulated
    filter is not available here: parity with librosa.load is UNPINNED (the mel front end is)."""
    if sr_in == sr_out:
        return x.astype(np.float32)
    g = math.gcd(sr_in, sr_out)
    up, down = sr_out // g, sr_in // g                      # output k sits at input time k * down / up
    cutoff = rolloff * min(1.0, sr_out / sr_in)
    half = int(math.ceil(num_zeros / cutoff))
    n_out = int(math.ceil(len(x) * sr_out / sr_in))
    taps = np.arange(-half + 1, half + 1)                   # input offsets around floor(t)
    phases = np.arange(up) * down % up / up                 # fractional part of t per phase
    t = taps[None, :] - phases[:, None]                     # [up, 2 half] distance input - t
    win = np.i0(beta * np.sqrt(np.clip(1.0 - (t / (half + 1)) ** 2, 0.0, 1.0))) / np.i0(beta)
    filt = (cutoff * np.sinc(cutoff * t) * win).astype(np.float64)
    xp = np.concatenate([np.zeros(half, np.float64), x.astype(np.float64), np.zeros(2 * half + 1, np.float64)])
    out = np.empty(n_out, np.float64)
    k = np.arange(n_out)
    base = (k * down) // up
    ph = k % up
    for s in range(0, n_out, 8192):
        e = min(n_out, s + 8192)
        idx = base[s:e, None] + half + taps[None, :]
        out[s:e] = np.einsum("ij,ij->i", xp[idx], filt[ph[s:e]])
    return out.astype(np.float32)


def load_wav(path: str, sr: int = 16000) -> np.ndarray:
    """librosa.load(path, sr=sr) for PCM .wav files: float32 mono (channels averaged) at ``sr``."""
    with wave.open(path, "rb") as w:
        ch, width, rate, n = w.getnchannels(), w.getsampwidth(), w.getframerate(), w.getnframes()
        raw = w.readframes(n)
    x = _pcm_to_float(raw, width).reshape(-1, ch).mean(axis=1)
    return resample(x, rate, sr)


# ----------------------------------------------------------------------------- video header
def mp4_video_info(path: str) -> dict:
    """Width, height, frame count and fps of the first video track of an MP4 (ISO BMFF boxes:
    tkhd, mdhd, hdlr, stts) — enough to size synthetic frames when no decoder exists."""
    with open(path, "rb") as f:
        data = f.read()
    tracks = []

    def walk(off, end, cur):
        while off + 8 <= end:
            size, typ = struct.unpack(">I4s", data[off:off + 8])
            hdr = 8
            if size == 1:
                size, hdr = struct.unpack(">Q", data[off + 8:off + 16])[0], 16
            elif size == 0:
                size = end - off
            if size < hdr:
                break
            body = data[off + hdr: off + size]
            t = typ.decode("latin1")
            if t == "trak":
                tr = {}
                tracks.append(tr)
                walk(off + hdr, off + size, tr)
            elif t in ("moov", "mdia", "minf", "stbl"):
                walk(off + hdr, off + size, cur)
            elif t == "tkhd" and cur is not None:
                v = body[0]
                o = 4 + (32 if v == 1 else 20) + 8 + 8 + 36
                cur["width"], cur["height"] = (struct.unpack(">I", body[o + k: o + k + 4])[0] / 65536.0 for k in (0, 4))
            elif t == "mdhd" and cur is not None:
                v = body[0]
                if v == 1:
                    cur["timescale"], cur["duration"] = struct.unpack(">IQ", body[20:32])
                else:
                    cur["timescale"], cur["duration"] = struct.unpack(">II", body[12:20])
            elif t == "hdlr" and cur is not None:
                cur["handler"] = body[8:12].decode("latin1")
            elif t == "stts" and cur is not None:
                n = struct.unpack(">I", body[4:8])[0]
                cur["frames"] = sum(struct.unpack(">I", body[8 + 8 * i: 12 + 8 * i])[0] for i in range(n))
            off += size

    walk(0, len(data), None)
    for tr in tracks:
        if tr.get("handler") == "vide":
            fps = tr["frames"] * tr["timescale"] / tr["duration"] if tr.get("duration") else 25.0
            return {"width": int(round(tr["width"])), "height": int(round(tr["height"])), "frames": tr["frames"],
                    "fps": fps}
    raise ValueError(f"{path}: no video track found")


# ----------------------------------------------------------------------------- runner
def _weights(ckpt_dir):
    from . import models, synth
    from .models import arch
    names = {k: os.path.join(ckpt_dir or "", f) for k, f in (("LNet", "LNet.pth"), ("ENet", "ENet.pth"),
                                                              ("DNet", "DNet.pt"))}
    if ckpt_dir and all(os.path.exists(p) for p in names.values()):
        args = argparse.Namespace(LNet_path=names["LNet"], ENet_path=names["ENet"], DNet_path=names["DNet"])
        return models.load_network(args), models.load_DNet(args), "checkpoints"
    enet = models.ENet(lnet=models.LNet())
    enet.load_state_dict(synth.synth_torch_state_dict(arch.ENetParams(lnet=arch.LNetParams())), strict=True)
    dnet = models.DNet()
    dnet.load_state_dict(synth.synth_torch_state_dict(arch.DNetParams()), strict=True)
    return enet.eval(), dnet.eval(), "synthetic"


def _frames(face: str, max_frames: int):
    from . import synth
    if face.endswith(".npy"):
        fr = np.load(face, allow_pickle=False)
        if fr.dtype != np.uint8 or fr.ndim != 4 or fr.shape[3] != 3:
            raise ValueError("--face .npy must hold uint8 [N,H,W,3] BGR frames")
        return fr[:max_frames], 25.0, "npy"
    info = mp4_video_info(face)
    n = min(info["frames"], max_frames)
    return synth.sr_frame(f"inference.{os.path.basename(face)}", n, info["height"], info["width"]), info["fps"], \
        f"synthetic {info['width']}x{info['height']} (no decoder; {info['frames']} frames in the file)"


def decode_jpeg_frames(files, dev, batch: int = 16, first: int = 0, jpeg_decode: str | None = "wave") -> torch.Tensor:
    """JPEG files of one size and sampling -> uint8 BGR [n, H, W, 3] on ``dev``, decoded there in batches of
    ``batch`` (mjpeg.JpegDecoder): the frames never exist on the host.  A damaged stream raises ValueError naming
    its frame (``first``: the number of files[0] in the clip).  ``jpeg_decode``: the decoder's ``split``
    (mjpeg.jpeg_decode_mode: "wave", "lane", "sync", "auto"; None reads S2V_JPEG_DECODE)."""
    from . import mjpeg
    info = mjpeg.parse_jpeg(files[0])
    dec = mjpeg.JpegDecoder(info.h, info.w, info.sampling, order="bgr", device=dev,
                            split=mjpeg.jpeg_decode_mode(jpeg_decode))
    out = torch.empty((len(files), info.h, info.w, 3), dtype=torch.uint8, device=dev)
    status = []
    for s in range(0, len(files), max(1, batch)):
        status.append(dec.decode(files[s:s + max(1, batch)], out=out[s:s + max(1, batch)])[1])
    bad = torch.cat(status).cpu().numpy()
    if bad.any():
        k = int(np.nonzero(bad)[0][0])
        raise ValueError(f"frame {first + k}: damaged JPEG stream (decoder status {int(bad[k])}; "
                         f"{int((bad != 0).sum())} of {len(files)} frames)")
    return out


# face3d's 5-point 3D reference when BFM/similarity_Lm3D_all.mat is absent (stated stand-in, the
# layout of lm3d_from_68: eyes, nose tip, mouth corners)
LM3D_STANDIN = np.array([[-0.31, 0.29, 0.41], [0.31, 0.29, 0.41], [0.0, 0.0, 0.65], [-0.25, -0.36, 0.44],
                         [0.25, -0.36, 0.44]])


def _lm3d(ckpt_dir):
    """face3d's 5-point 3D reference: BFM/similarity_Lm3D_all.mat under ``ckpt_dir``, else LM3D_STANDIN."""
    from . import face3d
    bfm = os.path.join(ckpt_dir or "", "BFM")
    return face3d.load_lm3d(bfm) if os.path.exists(os.path.join(bfm, "similarity_Lm3D_all.mat")) else LM3D_STANDIN


def _usable_landmarks(lms, H, W, lm3d):
    """Landmarks whose align_img fit s2v_pil_resize_crop cannot compute (an empty resized frame, a
    downscale past its 48-tap limit, sizes past int32: points that are no face, as synthetic FAN weights
    give) -> all -1,
    the reference's own marker of a frame without landmarks (facing.py:110-113).  Returns (landmarks,
    number of frames rejected); nothing is dropped silently, ``meta`` reports the count."""
    from . import face3d
    lms = np.array(lms, np.float32)
    rejects = 0
    for i in range(len(lms)):
        if np.mean(lms[i]) == -1:
            continue
        try:
            with np.errstate(all="ignore"):
                _, box, _ = face3d.align_params(W, H, face3d.frame_landmarks(lms[i], W, H, lm3d), lm3d)
            face3d._check_scale(W, H, box[0], box[1])
            if max(abs(v) for v in box) >= 1 << 31:          # the kernel's (w, h, left, up) are int32
                raise OverflowError(box)
        except (ValueError, OverflowError):                 # a degenerate fit: the scale is 0, inf or NaN
            lms[i] = -1.0
            rejects += 1
    return lms, rejects


def _semantic(frames_bgr: torch.Tensor, ckpt_dir, dev, lms=None, geometry="host"):
    """facing.py:100-130 face_3dmm_extraction on the frames: ReconNetWrapper('resnet50') from
    face3d_pretrain_epoch_20.pth (synthetic weights without it) -> [n, 262].  ``lms``: the frames' 68
    landmarks [n, 68, 2] (_landmarks); without them the reference's no-landmark path (all -1 landmarks ->
    lm3d positions, facing.py:110-116).  ``geometry`` "device": ``lms`` is a device tensor (_landmarks with
    on_device) and Face3DExtractor.semantic_device runs -> ((semantic [n, 262], status [n]) on the device, kind)."""
    from . import face3d, models, synth
    from .models.face3d_arch import ReconNetWrapperParams
    path = os.path.join(ckpt_dir or "", "face3d_pretrain_epoch_20.pth")
    if ckpt_dir and os.path.exists(path):
        net = models.load_face3d_net(path, dev)
        kind = "checkpoint"
    else:
        net = models.ReconNetWrapper()
        net.load_state_dict(synth.synth_torch_state_dict(ReconNetWrapperParams(), **synth.RETINA_SYNTH))
        net = net.eval()
        kind = "synthetic"
    lm3d = _lm3d(ckpt_dir)
    n = frames_bgr.shape[0]
    rgb = frames_bgr[..., [2, 1, 0]].contiguous()                               # facing.py reads RGB PIL frames
    ext = face3d.Face3DExtractor(net, lm3d, dev)
    if geometry == "device":
        if lms is None:
            lms = torch.full((n, 68, 2), -1.0, device=dev)
        return ext.semantic_device(rgb, lms), kind
    if lms is None:
        lms = np.full((n, 68, 2), -1.0, np.float32)
    return ext.face_3dmm_extraction(rgb, lms), kind


def _landmarks(frames_bgr: torch.Tensor, ckpt_dir, dev, detector=None, nms="host", on_device=False):
    """facing.py:89-97: KeypointExtractor().extract_keypoint on the RGB frames -> (landmarks [n, 68, 2],
    FAN weight kind, frames without a face).  FAN weights from <checkpoints>/2DFAN4.pth, or the synthetic
    FAN_SYNTH preset without it; the boxes come from the S3FD detector of _face_detector.  ``on_device``: the
    landmarks stay on the device (extract_keypoint_device), float32 [n, 68, 2]."""
    from . import face3d
    if detector is None:
        detector, kind = _landmark_detector(ckpt_dir, dev, nms)
    else:
        kind = "given detector"
    kp = face3d.KeypointExtractor(detector)
    if on_device:
        return kp.extract_keypoint_device(frames_bgr[..., [2, 1, 0]].contiguous()), kind, kp.misses
    lms = kp.extract_keypoint(frames_bgr[..., [2, 1, 0]].contiguous(), info=False)
    return lms.astype(np.float32), kind, kp.misses


def _landmark_detector(ckpt_dir, dev, nms="host"):
    """KeypointExtractor's detector: FaceAlignment over S3FD (_face_detector) with the FAN weights of
    <checkpoints>/2DFAN4.pth, or the synthetic FAN_SYNTH preset without it -> (detector, FAN weight kind)."""
    from . import models, synth
    from .models.fan_arch import FANParams
    path = os.path.join(ckpt_dir or "", "2DFAN4.pth")
    if ckpt_dir and os.path.exists(path):
        fan, kind = models.load_fan(path), "2DFAN4 checkpoint"
    else:
        fan = models.FAN()
        fan.load_state_dict(synth.synth_torch_state_dict(FANParams(), **synth.FAN_SYNTH), strict=True)
        fan, kind = fan.eval(), "2DFAN4 synthetic"
    detector, _ = _face_detector(ckpt_dir, dev, nms)
    detector.face_alignment_net = fan
    return detector, kind


class BoxedStitch:
    """datagen's references for ``run`` (inference.py:359-367): stitch.Stitcher on each batch, then the pasted
    256 x 256 image resized into the frame's face box and the reference cut there again (:364-367).  In ``run``
    the paste box and the face_detect box are one box, so that is cv2.resize to the box size and back: the
    references carry the same two resamplings.  ``boxes``: (y1, y2, x1, x2) per frame of the clip, taken in
    call order."""

    def __init__(self, stitcher, boxes):
        self.stitcher, self.boxes, self.k = stitcher, list(boxes), 0

    @property
    def misses(self):
        return self.stitcher.misses

    def __call__(self, ref_u8, base_u8):
        from . import post
        out = self.stitcher(ref_u8, base_u8).permute(0, 2, 3, 1).contiguous()
        h, w = out.shape[1:3]
        for i in range(out.shape[0]):
            y1, y2, x1, x2 = self.boxes[self.k]
            self.k += 1
            boxed = post.resize_linear(out[i], (x2 - x1, y2 - y1))
            post.resize_linear(boxed, (w, h), out=out[i])
        return out.permute(0, 3, 1, 2).contiguous()


def _face_detector(ckpt_dir, dev, nms="host"):
    """face_detect's default detector (inference_utils.py:111-113): FaceAlignment(_2D) over S3FD with the
    weights of <checkpoints>/s3fd.pth, or the synthetic preset without it -> (detector, weight kind).
    ``nms``: SFDDetector's ("host" / "device")."""
    from . import face_detection, models, synth
    from .models.s3fd_arch import S3FDParams
    path = os.path.join(ckpt_dir or "", "s3fd.pth")
    if ckpt_dir and os.path.exists(path):
        net, kind = models.load_s3fd(path), "s3fd checkpoint"
    else:
        net = models.S3FD()
        net.load_state_dict(synth.s3fd_state_dict(S3FDParams()), strict=True)
        net, kind = net.eval(), "s3fd synthetic"
    sfd = face_detection.SFDDetector(dev, net=net, nms=nms)
    return face_detection.FaceAlignment(face_detection.LandmarksType._2D, device=dev, flip_input=False,
                                        detector=sfd), kind


def _up_face_model(ckpt_dir, dev):
    """inference.py:250-253: GANimationModel().initialize() / setup() with the generator of
    <checkpoints>/30_net_gen.pth, or the synthetic GANIMATION_SYNTH preset without it -> (model, weight kind)."""
    from . import ganimation, models, synth
    path = os.path.join(ckpt_dir or "", ganimation.CKPT_NAME)
    if ckpt_dir and os.path.exists(path):
        net, kind = models.load_ganimation(path), "30_net_gen checkpoint"
    else:
        net = models.SplitGenerator()
        net.load_state_dict(synth.synth_torch_state_dict(net, **synth.GANIMATION_SYNTH), strict=True)
        net, kind = net.eval(), "30_net_gen synthetic"
    return ganimation.GANimationModel().initialize(net_gen=net, device=dev).setup(), kind


def _ref_enhancer(ckpt_dir, dev, nms="host"):
    """inference.py:224-226: FaceEnhancement(in_size=512, channel_multiplier=2, narrow=1, sr_scale=4,
    model='GPEN-BFR-512', use_sr=False) as a hook on the stabilised uint8 RGB references."""
    from . import face as faces
    base = ckpt_dir or "checkpoints"
    enh = faces.FaceEnhancement(base_dir=base, in_size=512, channel_multiplier=2, narrow=1, sr_scale=4,
                                model="GPEN-BFR-512", use_sr=False, device=dev,
                                facedetector=faces.RetinaFaceDetection(base, dev, nms=nms))
    return reference_hook(enh)


def reference_hook(enh):
    """Step 5 (inference.py:234-238) as a LipSyncPipeline ref hook: each uint8 RGB [3, h, w] reference
    -> BGR HWC -> ``enh.process_device(img, img, face_enhance=False, possion_blending=False)`` -> back."""
    def hook(ref_u8: torch.Tensor) -> torch.Tensor:
        out = torch.empty_like(ref_u8)
        for i in range(ref_u8.shape[0]):
            bgr = ref_u8[i].flip(0).permute(1, 2, 0).contiguous()
            img = enh.process_device(bgr, bgr, face_enhance=False, possion_blending=False)[0]
            out[i] = img.permute(2, 0, 1).flip(0)
        return out
    return hook


def run(face: str, audio_path: str, max_frames: int = 8, batch: int = 16, box_frac: float = 0.6,
        ckpt_dir: str | None = None, enhance: bool = False, device: str = "cuda", ref_enhance: bool = False,
        ref_hook=None, restore: bool = True, restorer=None, enhancer=None, face_det: bool = False,
        pads=(0, 20, 0, 0), nosmooth: bool = False, face_det_batch_size: int = 4, detector=None,
        landmarks: bool = False, landmark_detector=None, stitch: bool = False, stitch_detector=None,
        up_face: str = "original", without_rl1: bool = False, up_face_model=None, precision: str | None = None,
        nms: str | None = "host", fps: float = 25.0, jpeg_decode: str | None = "wave",
        audio_load: str | None = "host", geometry: str | None = "host"):
    """-> dict(frames uint8 [n,H,W,3] device, preds uint8 [n,3,384,384], meta).  ``ref_enhance``:
    Step 5 with FaceEnhancement-512 (``ref_hook``: any callable on uint8 [b,3,h,w] references).
    ``enhance``: the per-frame tail of inference.py:296-330 on the pasted frames -> ``enhanced``
    uint8 [n,2H,2W,3]: GFPGANer.enhance(ff, only_center_face=True) (``restore``; restore.GFPGANer,
    :300-301), the FaceParse mouth mask + 10-level Laplacian blend (post.MouthBlend, :302-313), then
    FaceEnhancement-2048 with SR x2 on the 2x frame (:326-327).  ``restorer`` / ``enhancer``: given
    objects (else built from ``ckpt_dir`` as the reference builds them).  ``face_det``: per-frame face
    boxes from face_detection.face_detect(frames, pads, nosmooth, jaw_correction=True,
    face_det_batch_size) instead of the centred square; they drive the DNet crop, the paste-back, the mouth
    blend and FaceEnhancement's bbox, and ``meta`` gains ``boxes`` / ``box_source``.  ``detector``: an
    object with get_detections_for_batch (else S3FD from ``ckpt_dir``/s3fd.pth, or synthetic weights).
    ``landmarks``: the frames' 68 FAN landmarks (_landmarks; ``landmark_detector``: an object with
    get_landmarks_from_batch) drive the 3DMM extraction instead of the no-landmark path; ``meta`` gains
    ``landmarks`` (the FAN weight kind), ``landmark_misses`` (frames without a face) and ``landmark_rejects``
    (_usable_landmarks), the result gains ``semantic`` [n, 262].  ``stitch``: datagen's reference stitch
    (stitch.Stitcher through BoxedStitch) on the stabilised references, over ``stitch_detector`` (an object with
    get_landmarks_from_batch; else S3FD + FAN from ``ckpt_dir`` or the synthetic presets, whose points are no
    face: a frame with an unusable quad raises ValueError); ``meta`` gains ``stitch``, ``stitch_misses`` (frames
    without a face, which reuse their predecessor's points) and ``stitch_landmarks`` (the FAN weight kind).
    ``up_face`` ('original', 'sad', 'angry', 'surprise') / ``without_rl1``: GANimation's upper-face edit and the
    composite of inference.py:269-286 (``up_face_model``: an initialised ganimation.GANimationModel, else one
    over ``ckpt_dir``/30_net_gen.pth or the synthetic preset); ``meta`` gains ``up_face``, ``without_rl1`` and
    ``up_face_weights``.  ``precision``: the conv arithmetic of the whole clip (an ops.set_precision name; None
    leaves ops.PRECISION alone), restored afterwards; ``meta["conv_arith"]`` names the arithmetic that ran.  The
    opt-in "f16" (single-pass f16 products) is outside the fp32 parity bar: about 0.5 grey level on average.
    ``nms``: where the greedy NMS of every detector this call builds runs (S3FD, and RetinaFace in
    FaceEnhancement and GFPGANer): "host" (the default), "device" (face.nms_device; equal scores take the larger
    position index first) or None for S2V_NMS; given detectors keep their own.  ``meta["nms"]`` records it.
    ``face``: NAME.avi (Motion-JPEG: the frames are decoded on the device in batches of ``batch`` and stay there, fps
    from the header, ``meta["video"]`` "avi mjpeg WxH"; a damaged frame raises ValueError naming it), NAME.jpg /
    .jpeg (the reference's static mode: the one frame for every mel window up to ``max_frames``, at ``fps``), an MP4
    (header only: synthetic frames) or an .npy array.  ``fps`` is used for a static image only.  ``jpeg_decode``:
    how the entropy stage of the JPEG decoder is split: "wave" (the default), "lane", "sync" (parallel inside an
    interval: for files without restart markers, which is what ffmpeg and Pillow write), "auto" or None for
    S2V_JPEG_DECODE; ``meta["jpeg_decode"]`` records it.  ``audio_load``: where ``audio_path`` becomes float32 mono
    at 16 kHz: "host" (the default: load_wav, stdlib ``wave`` + NumPy), "device" (audio.load_audio: the file's sample
    bytes are decoded, downmixed and resampled in one launch; it also reads IEEE-float and EXTENSIBLE files, which
    ``wave`` refuses) or None for S2V_AUDIO_LOAD; ``meta["audio_load"]`` records it.  ``geometry``: where the
    arithmetic between the preprocessing networks runs: "host" (the default), "device" or None for S2V_GEOMETRY.
    With "device" the landmarks' map back to the frame (s2v_fan_landmarks), align_img's parameters with the
    validation of _usable_landmarks (s2v_face3d_align; ``landmark_rejects`` counts its status 2) and the DNet
    coefficient windows (s2v_dnet_windows) run there, and ``semantic`` comes to the host once, at the end;
    ``stitch`` keeps reading its own landmarks through the host.  ``meta["geometry"]`` records it."""
    kw = dict(locals())                                     # the arguments (nothing else is bound yet)
    from . import audio, mjpeg, ops, pipeline, post, synth
    from . import face as faces
    nms = kw["nms"] = faces.nms_mode(nms)                   # ValueError on a bad name before anything runs
    jpeg_decode = kw["jpeg_decode"] = mjpeg.jpeg_decode_mode(jpeg_decode)           # likewise
    audio_load = kw["audio_load"] = audio.audio_load_mode(audio_load)               # likewise
    from . import face3d
    geometry = kw["geometry"] = face3d.geometry_mode(geometry)                      # likewise
    if precision is not None:
        kw["precision"] = None
        with ops.precision(precision):                      # ValueError on a bad name before anything runs
            return run(**kw)
    if up_face != "original":
        from . import ganimation
        ganimation.check_up_face(up_face)                  # ValueError before anything runs
    dev = torch.device(device)
    t0 = time.time()
    kind = os.path.splitext(face)[1].lower()
    if kind == ".avi":
        from . import mjpeg
        reader = mjpeg.AviReader(face)                     # ValueError on a codec that is not Motion-JPEG
        fps, available = reader.fps, min(len(reader), max_frames)
    elif kind in (".jpg", ".jpeg"):
        available = max_frames                             # the reference's static mode (inference.py:58-64, :371)
    else:
        frames_np, fps, src_kind = _frames(face, max_frames)
        available = len(frames_np)
    if audio_load == "device":
        wav = audio.load_audio(audio_path, 16000, dev)
        mel = audio.melspectrogram(wav)
    else:
        wav = load_wav(audio_path, 16000)
        mel = audio.melspectrogram(torch.from_numpy(wav).to(dev))
    chunks = audio.mel_chunks(mel, fps=fps)
    n = min(available, chunks.shape[0])                                             # inference.py:219-221
    if kind == ".avi":
        if n == 0:
            raise ValueError(f"{face}: no frames")
        frames = decode_jpeg_frames(reader.frames(0, n), dev, batch, jpeg_decode=jpeg_decode)
        src_kind = f"avi mjpeg {frames.shape[2]}x{frames.shape[1]}"
    elif kind in (".jpg", ".jpeg"):
        with open(face, "rb") as f:
            one = decode_jpeg_frames([f.read()], dev, jpeg_decode=jpeg_decode)
        frames = one.repeat(n, 1, 1, 1)                                             # one frame for every window
        src_kind = f"jpeg {one.shape[2]}x{one.shape[1]} (static)"
    else:
        frames = torch.from_numpy(np.ascontiguousarray(frames_np[:n])).to(dev)
    H, W = frames.shape[1:3]
    side = int(min(H, W) * box_frac)
    y1, x1 = (H - side) // 2, (W - side) // 2
    y2, x2 = y1 + side, x1 + side
    boxes, box_source = [(y1, y2, x1, x2)] * n, None
    if face_det:
        from . import face_detection
        if detector is None:
            detector, box_source = _face_detector(ckpt_dir, dev, nms)
        else:
            box_source = "given detector"
        det = face_detection.face_detect(frames, pads=pads, nosmooth=nosmooth, jaw_correction=True,
                                         batch_size=face_det_batch_size, detector=detector)   # inference.py:357
        boxes = [tuple(int(v) for v in c) for _, c in det]
        if any(b[1] <= b[0] or b[3] <= b[2] for b in boxes):
            raise ValueError(f"face_detect: empty face box among {boxes}")
    enet, dnet, wkind = _weights(ckpt_dir)
    # DNet source: trans_image of the box crop (256x256, ToTensor + Normalize(0.5, 0.5), RGB)
    crops = torch.empty((n, 256, 256, 3), dtype=torch.uint8, device=dev)
    for i, (by1, by2, bx1, bx2) in enumerate(boxes):
        post.resize_linear(frames[i, by1:by2, bx1:bx2], (256, 256), out=crops[i])
    src = torch.empty((n, 3, 256, 256), device=dev)
    ctx = post._ctx(dev)
    from ._lib import check
    check(ctx.lib.s2v_u8_to_gan(crops.data_ptr(), n, 256, 256, src.data_ptr(), ctx.stream), "s2v_u8_to_gan")
    lms = None
    expression = synth.hash_array("inference.expression", (64,), -1.0, 1.0)        # expression.mat is absent
    if geometry == "device":
        if landmarks:
            lms, lkind, lmiss = _landmarks(frames, ckpt_dir, dev, landmark_detector, nms, on_device=True)
        (semantic_dev, fit_status), skind = _semantic(frames, ckpt_dir, dev, lms, geometry)
        coeffs = pipeline.dnet_coefficients_device(semantic_dev, expression, False, 0, n)
    else:
        if landmarks:
            lms, lkind, lmiss = _landmarks(frames, ckpt_dir, dev, landmark_detector, nms)   # facing.py:89-97
            lms, lrej = _usable_landmarks(lms, H, W, _lm3d(ckpt_dir))
        semantic, skind = _semantic(frames, ckpt_dir, dev, lms)                    # facing.py:100-130
        coeffs = torch.from_numpy(pipeline.dnet_coefficients(semantic, expression, False, 0, n)).to(dev)
    if ref_enhance and ref_hook is None:
        ref_hook = _ref_enhancer(ckpt_dir, dev, nms)
    stitcher = None
    if stitch:
        from . import face3d
        from . import stitch as stitching
        if stitch_detector is None:
            stitch_detector, stkind = _landmark_detector(ckpt_dir, dev, nms)
        else:
            stkind = "given detector"
        stitcher = BoxedStitch(stitching.Stitcher(face3d.KeypointExtractor(stitch_detector), image_size=256), boxes)
    ukind = None
    if up_face != "original" and up_face_model is None:
        up_face_model, ukind = _up_face_model(ckpt_dir, dev)                        # inference.py:250-253
    elif up_face != "original":
        ukind = "given model"
    orig = None
    if without_rl1:
        # img_original (inference.py:384, :396): cv2.resize(oface, (img_size, img_size)), in the predictions' RGB
        orig = torch.empty((n, 384, 384, 3), dtype=torch.uint8, device=dev)
        for i, (by1, by2, bx1, bx2) in enumerate(boxes):
            post.resize_linear(frames[i, by1:by2, bx1:bx2], (384, 384), out=orig[i])
        orig = orig[..., [2, 1, 0]].contiguous()
    pipe = pipeline.LipSyncPipeline(dnet, enet, device=dev, batch=batch, graph=False, ref_hook=ref_hook,
                                    stitch=stitcher, up_face=up_face_model if up_face != "original" else None,
                                    up_face_name=up_face if up_face != "original" else None,
                                    without_rl1=without_rl1)
    preds = pipe.run(chunks[:n], src, coeffs, orig_u8=orig)                         # [n,3,384,384] uint8
    out = frames.clone()
    hwc = preds.permute(0, 2, 3, 1).contiguous()
    for i, (by1, by2, bx1, bx2) in enumerate(boxes):                                # inference.py:287-291
        post.resize_linear(hwc[i], (bx2 - bx1, by2 - by1), out=out[i, by1:by2, bx1:bx2])
    enhanced = None
    if enhance:
        base = ckpt_dir or "checkpoints"
        enh = enhancer or faces.FaceEnhancement(base_dir=base, in_size=2048, channel_multiplier=2, narrow=1,
                                                sr_scale=2, sr_model=None, model="GPEN-BFR-2048", use_sr=True,
                                                device=device,                       # inference.py:228-231
                                                facedetector=faces.RetinaFaceDetection(base, device, nms=nms))
        if restore and restorer is None:
            from .restore import GFPGANer, RetinaFaceDetector
            restorer = GFPGANer(model_path=os.path.join(base, "GFPGANv1.4.pth"), upscale=1, arch="clean",
                                channel_multiplier=2, bg_upsampler=None, device=device, base_dir=base,
                                face_det=RetinaFaceDetector(base, device, nms=nms))   # :255-256
        mouth = post.MouthBlend(enh.faceparser)
        enhanced = []
        for i in range(n):
            pp, box = out[i], boxes[i]
            if restore:
                _, _, restored_img = restorer.enhance(pp, has_aligned=False, only_center_face=True,
                                                      paste_back=True)                  # inference.py:300-301
                pp = mouth.run(restored_img, pp, box)                                   # :302-313
            big = post.resize_linear(frames[i], (2 * W, 2 * H))                      # tmp_xf (inference.py:326)
            enhanced.append(enh.process_device(pp, big, bbox=box, face_enhance=True, possion_blending=True)[0])
        enhanced = torch.stack(enhanced)
    torch.cuda.synchronize(dev)
    meta = {"frames": n, "frame_hw": [int(H), int(W)], "fps": fps, "video": src_kind, "weights": wkind,
            "mel_cols": int(mel.shape[1]), "mel_windows": int(chunks.shape[0]), "wav_samples_16k": int(len(wav)),
            "box": [y1, y2, x1, x2], "semantic": skind, "ref_enhance": ref_hook is not None,
            "restore": bool(enhance and restore), "up_face": up_face, "without_rl1": bool(without_rl1),
            "up_face_weights": ukind, "conv_arith": ops.PRECISION, "nms": nms, "jpeg_decode": jpeg_decode,
            "audio_load": audio_load, "geometry": geometry,
            "seconds": round(time.time() - t0, 3)}
    if face_det:
        meta["boxes"] = [list(b) for b in boxes]
        meta["box_source"] = box_source
    if stitch:
        meta["stitch"] = True
        meta["stitch_misses"] = int(stitcher.misses)
        meta["stitch_landmarks"] = stkind
    res = {"frames": out, "preds": preds, "enhanced": enhanced, "meta": meta}
    if landmarks and geometry == "device":                 # the one copy of the device route's results
        semantic = semantic_dev.cpu().numpy()
        lrej = int((fit_status == face3d.ALIGN_REJECTED).sum().item())
    if landmarks:
        meta["landmarks"] = lkind
        meta["landmark_misses"] = int(lmiss)
        meta["landmark_rejects"] = int(lrej)
        res["semantic"] = semantic
    return res


def build_parser():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--face", required=True,
                    help="Motion-JPEG .avi (decoded on the device), one .jpg / .jpeg (static: the frame repeats), MP4 "
                         "(header read; synthetic frames) or uint8 [N,H,W,3] .npy")
    ap.add_argument("--fps", type=float, default=25.0, help="with --face NAME.jpg: frames per second of the clip")
    ap.add_argument("--audio", required=True,
                    help="PCM .wav (8/16/24/32 bit); with --audio_load device also IEEE-float (32/64 bit) and "
                         "WAVE_FORMAT_EXTENSIBLE files; any rate and channel count: averaged to mono, resampled to "
                         "16 kHz")
    ap.add_argument("--outfile", default="results/inference_frames.npz",
                    help="NAME.avi: a Motion-JPEG AVI of the frames (the --enhance output when there is one) with the "
                         "audio of --audio; anything else: the uint8 arrays as a compressed .npz")
    ap.add_argument("--max_frames", type=int, default=8)
    ap.add_argument("--LNet_batch_size", type=int, default=16)
    ap.add_argument("--box_frac", type=float, default=0.6)
    ap.add_argument("--checkpoints", default=None)
    ap.add_argument("--enhance", action="store_true")
    ap.add_argument("--no_restore", action="store_true", help="with --enhance: skip GFPGANer + the mouth blend")
    ap.add_argument("--ref_enhance", action="store_true", help="Step 5: FaceEnhancement-512 on the references")
    ap.add_argument("--face_det", action="store_true", help="per-frame face boxes from S3FD (face_detect)")
    ap.add_argument("--pads", nargs="+", type=int, default=[0, 20, 0, 0],
                    help="with --face_det: padding (top, bottom, left, right) of the detected box")
    ap.add_argument("--nosmooth", action="store_true", help="with --face_det: no 5-frame smoothing of the boxes")
    ap.add_argument("--face_det_batch_size", type=int, default=4, help="with --face_det: frames per detector batch")
    ap.add_argument("--landmarks", action="store_true",
                    help="68 FAN landmarks per frame (S3FD + 2DFAN4) drive the 3DMM extraction")
    ap.add_argument("--stitch", action="store_true",
                    help="datagen's reference stitch: quad crop of each stabilised reference pasted over the original "
                         "crop (needs real S3FD / FAN weights: synthetic ones give points that are no face, and a "
                         "frame with an unusable quad raises)")
    ap.add_argument("--up_face", default="original",
                    help="upper-face expression edit by GANimation: original (none), sad, angry or surprise; it "
                         "reaches the frames only with --without_rl1")
    ap.add_argument("--without_rl1", default=False, action="store_true",
                    help="composite the (edited) original crop over the prediction wherever the masked input was "
                         "not zero: the upper half of the face")
    ap.add_argument("--precision", default=None, choices=["f16x3", "bf16x3", "f32", "f16"],
                    help="conv arithmetic of the whole clip (default: the process setting, S2V_PRECISION or f16x3); "
                         "f16 is the fast single-pass mode, OUTSIDE the fp32 parity bar (about 0.5 grey level on "
                         "average, 3-5 at the worst pixel)")
    ap.add_argument("--nms", default=None, choices=["host", "device"],
                    help="where every detector's greedy NMS runs (default: S2V_NMS, else host); device: the "
                         "batched kernel, equal scores take the larger position index first")
    ap.add_argument("--jpeg_decode", default=None, choices=["wave", "lane", "sync", "auto"],
                    help="with --face NAME.avi / .jpg: the split of the JPEG decoder's entropy stage (default: "
                         "S2V_JPEG_DECODE, else wave); sync decodes inside a restart interval in parallel, for files "
                         "without restart markers (ffmpeg's and Pillow's); auto picks sync for long intervals")
    ap.add_argument("--audio_load", default=None, choices=["host", "device"],
                    help="where --audio is decoded, downmixed and resampled to 16 kHz (default: S2V_AUDIO_LOAD, else "
                         "host); device: one kernel launch on the file's sample bytes")
    ap.add_argument("--geometry", default=None, choices=["host", "device"],
                    help="where the arithmetic between the preprocessing networks runs: the landmarks' map back to "
                         "the frame, align_img's parameters and their validation, the DNet coefficient windows "
                         "(default: S2V_GEOMETRY, else host); device: three small kernels, no per-point or per-frame "
                         "host work")
    ap.add_argument("--jpeg_quality", type=int, default=95,
                    help="with --outfile NAME.avi: JPEG quality 1..100 (the reference asks ffmpeg for its best, -q:v 1)")
    return ap


def write_avi(path: str, frames: torch.Tensor, fps: float, audio_path: str, quality: int = 95, batch: int = 16,
              audio_load: str | None = "host") -> int:
    """The reference's cv2.VideoWriter + ffmpeg mux (inference.py:246-249, :325-336) as one Motion-JPEG AVI:
    uint8 BGR [n, H, W, 3] device frames through mjpeg.JpegEncoder in batches of ``batch``, with the PCM of
    ``audio_path`` at its own rate and channel count, cut to the clip.  ``audio_load`` "device" (None: S2V_AUDIO_LOAD)
    takes the PCM from audio.pcm16, which also converts the float files load_audio reads; "host" from
    mjpeg.wav_pcm16.  -> the file's size in bytes."""
    from . import audio, mjpeg
    pcm = audio.pcm16(audio_path) if audio.audio_load_mode(audio_load) == "device" else mjpeg.wav_pcm16(audio_path)
    n, H, W = frames.shape[:3]
    enc = mjpeg.JpegEncoder(H, W, quality=quality, order="bgr", device=frames.device)
    with mjpeg.AviWriter(path, W, H, fps, audio=pcm) as avi:
        for s in range(0, n, max(1, batch)):
            for data in enc.encode_to_host(frames[s:s + max(1, batch)]):
                avi.write(data)
    return os.path.getsize(path)


def main(argv=None):
    a = build_parser().parse_args(argv)
    if len(a.pads) != 4:
        raise SystemExit("--pads takes four integers: top bottom left right")
    if a.outfile.lower().endswith(".avi") and not 1 <= a.jpeg_quality <= 100:
        raise SystemExit("--jpeg_quality takes 1 to 100")
    r = run(a.face, a.audio, a.max_frames, a.LNet_batch_size, a.box_frac, a.checkpoints, a.enhance,
            ref_enhance=a.ref_enhance, restore=not a.no_restore, face_det=a.face_det, pads=tuple(a.pads),
            nosmooth=a.nosmooth, face_det_batch_size=a.face_det_batch_size, landmarks=a.landmarks,
            stitch=a.stitch, up_face=a.up_face, without_rl1=a.without_rl1, precision=a.precision,
            nms=a.nms, fps=a.fps, jpeg_decode=a.jpeg_decode, audio_load=a.audio_load,
            geometry=a.geometry)
    os.makedirs(os.path.dirname(os.path.abspath(a.outfile)), exist_ok=True)
    if a.outfile.lower().endswith(".avi"):
        video = r["enhanced"] if r["enhanced"] is not None else r["frames"]
        size = write_avi(a.outfile, video, r["meta"]["fps"], a.audio, a.jpeg_quality, a.LNet_batch_size,
                         audio_load=r["meta"]["audio_load"])
        print(json.dumps(dict(r["meta"], outfile=a.outfile, video_bytes=size, jpeg_quality=a.jpeg_quality)))
        return 0
    arrays = {"frames": r["frames"].cpu().numpy(), "preds": r["preds"].cpu().numpy()}
    if r["enhanced"] is not None:
        arrays["enhanced"] = r["enhanced"].cpu().numpy()
    if "semantic" in r:
        arrays["semantic"] = r["semantic"]
    np.savez_compressed(a.outfile, **arrays)
    print(json.dumps(dict(r["meta"], outfile=a.outfile)))
    return 0


if __name__ == "__main__":
    sys.exit(main())
