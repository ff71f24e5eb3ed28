"""Device mel front end (reference futils/audio.py:45-51 with futils/hparams.py:21-61) and the
per-frame 16-column mel windows (inference.py:209-216), on libs2v kernels.

    mel = melspectrogram(wav_cuda)                 # [80, 1 + N//200] float32 on the device
    chunks = mel_chunks(mel, fps=25)               # [n_frames, 1, 80, 16] (LNet audio input)

Constant tables (Slaney mel basis, DFT twiddles, periodic Hann window) are built once on the host
in float64 and uploaded as float32.  pad_mode: 'constant' (librosa 0.9.2 stft default, the
pinned reference version) or 'reflect' (librosa <= 0.8).

The opt-in device loader in front of it (``audio_load_mode`` "device"; the default stays inference.load_wav):

    wav = load_audio("voice.wav", 16000)           # float32 [n] on the device, what inference.load_wav computes

``read_wav`` reads the RIFF/WAVE container itself (PCM 8/16/24/32 bit, IEEE float 32/64, EXTENSIBLE headers: more
than the stdlib ``wave`` opens), the sample bytes go to the device as they lie in the file, and one launch of
s2v_audio_load decodes, downmixes and resamples them with the filter of inference.resample (``resample_table``).
"""
from __future__ import annotations

import math
import os
import struct

import numpy as np
import torch

from . import _lib, ops
from .ops import Ctx

SR, N_FFT, HOP, N_MELS, FMIN, FMAX = 16000, 800, 200, 80, 55.0, 7600.0
_TABLES = {}
_CTX = {}


def _hz_to_mel(f):
    f = np.asanyarray(f, dtype=np.float64)
    f_sp, min_log_hz = 200.0 / 3, 1000.0
    logstep = np.log(6.4) / 27.0
    return np.where(f >= min_log_hz, min_log_hz / f_sp + np.log(np.maximum(f, 1e-12) / min_log_hz) / logstep, f / f_sp)


def _mel_to_hz(m):
    m = np.asanyarray(m, dtype=np.float64)
    f_sp, min_log_hz = 200.0 / 3, 1000.0
    min_log_mel = min_log_hz / f_sp
    logstep = np.log(6.4) / 27.0
    return np.where(m >= min_log_mel, min_log_hz * np.exp(logstep * (m - min_log_mel)), f_sp * m)


def slaney_mel_basis() -> np.ndarray:
    """[80, 401] float32 triangular Slaney-normalised filterbank (sr 16 kHz, 55..7600 Hz)."""
    freqs = np.fft.rfftfreq(n=N_FFT, d=1.0 / SR)
    edges = _mel_to_hz(np.linspace(_hz_to_mel(FMIN), _hz_to_mel(FMAX), N_MELS + 2))
    widths = np.diff(edges)
    w = np.zeros((N_MELS, freqs.size), dtype=np.float32)
    for i in range(N_MELS):
        rise = (freqs - edges[i]) / widths[i]
        fall = (edges[i + 2] - freqs) / widths[i + 1]
        w[i] = np.maximum(0.0, np.minimum(rise, fall))
    w *= (2.0 / (edges[2:] - edges[:-2]))[:, None]
    return w


def tables(device) -> torch.Tensor:
    key = str(device)
    if key not in _TABLES:
        k = np.arange(N_FFT, dtype=np.float64)
        ang = 2.0 * np.pi * k / N_FFT
        win = 0.5 - 0.5 * np.cos(ang)
        t = np.concatenate([slaney_mel_basis().astype(np.float64).ravel(), np.cos(ang), np.sin(ang), win])
        _TABLES[key] = torch.from_numpy(t.astype(np.float32)).to(device)
    return _TABLES[key]


def _ctx(device):
    key = str(device)
    if key not in _CTX:
        _CTX[key] = Ctx(device)
    return _CTX[key]


def melspectrogram(wav: torch.Tensor, pad_mode: str = "constant") -> torch.Tensor:
    """wav: 1-D float32 device tensor (16 kHz) -> [80, 1 + len//200] float32."""
    if not wav.is_cuda:
        raise _lib.S2VError("melspectrogram runs on the HIP device only")
    wav = wav.contiguous().float()
    n = wav.numel()
    frames = 1 + n // HOP
    out = torch.empty((N_MELS, frames), device=wav.device)
    ops.S2V.melspectrogram_(wav, tables(wav.device), pad_mode == "reflect", out)
    return out


def chunk_starts(n_cols: int, fps: float = 25.0, step: int = 16):
    """inference.py:209-216 window starts (host logic, integer)."""
    starts, i, mult = [], 0, 80.0 / fps
    while True:
        s = int(i * mult)
        if s + step > n_cols:
            starts.append(n_cols - step)
            return starts
        starts.append(s)
        i += 1


def mel_chunks(mel: torch.Tensor, fps: float = 25.0, step: int = 16) -> torch.Tensor:
    """[80, T] device mel -> [n, 1, 80, step] windows (the LNet audio input layout)."""
    T = mel.shape[1]
    st = chunk_starts(T, fps, step)
    starts = torch.tensor(st, dtype=torch.int32).to(mel.device)
    out = torch.empty((len(st), 1, N_MELS, step), device=mel.device)
    ops.S2V.mel_chunks_(mel.contiguous(), starts, step, out)
    return out


# ----------------------------------------------------------------------------- device audio loader
AUDIO_LOAD_MODES = ("host", "device")
AUDIO_LOAD_ENV = "S2V_AUDIO_LOAD"
PCM_BYTES = (1, 2, 3, 4, 4, 8)                  # per sample, by _lib.PCM_* format
TABLE_MAX_FLOATS = 1 << 24                      # up * row_stride of a resampling table (64 MiB)
_WAV_PCM, _WAV_FLOAT, _WAV_EXTENSIBLE = 1, 3, 0xFFFE
_WAV_COMPRESSED = {2: "MS ADPCM", 6: "A-law", 7: "\u00b5-law", 0x11: "IMA ADPCM", 0x31: "GSM 6.10", 0x50: "MPEG",
                   0x55: "MP3"}
KAISER_BEST = (64, 0.9475937167399596, 14.769656459379492)     # num_zeros, rolloff, beta: inference.resample's defaults
_RESAMPLE = {}
_RESAMPLE_DEV = {}


def audio_load_mode(name="host") -> str:
    """The ``audio_load=`` argument of inference.run: "host" (the default: inference.load_wav) or "device"
    (load_audio); None reads S2V_AUDIO_LOAD (unset or empty: "host").  Anything else raises ValueError."""
    source = "audio_load="
    if name is None:
        name, source = os.environ.get(AUDIO_LOAD_ENV) or "host", AUDIO_LOAD_ENV + "="
    if name not in AUDIO_LOAD_MODES:
        raise ValueError(f"{source}{name!r}: {AUDIO_LOAD_ENV} / audio_load= takes one of "
                         f"{', '.join(AUDIO_LOAD_MODES)}")
    return name


def read_wav(path: str):
    """-> (the interleaved little-endian sample bytes as a memoryview of whole frames, rate, channels,
    format (_lib.PCM_*), n_frames) of a RIFF/WAVE file: ``fmt`` tag 1 (PCM, 8/16/24/32 bit), 3 (IEEE float,
    32/64 bit) or 0xFFFE (EXTENSIBLE: the tag is the first two bytes of the sub-format GUID).  Chunks that are
    neither ``fmt `` nor ``data`` are skipped, with the pad byte after an odd size; a ``data`` size of 0xFFFFFFFF or
    past the end of the file (a stream written into a pipe) means "to the end of the file".  Anything else raises
    ValueError naming the file and the reason."""
    with open(path, "rb") as f:
        data = bytearray(os.fstat(f.fileno()).st_size)
        data = memoryview(data)[:f.readinto(data)]
    if len(data) < 12 or data[0:4] != b"RIFF" or data[8:12] != b"WAVE":
        raise ValueError(f"{path}: not a RIFF/WAVE file")
    fmt, off = None, 12
    while off + 8 <= len(data):
        cid, size = bytes(data[off:off + 4]), struct.unpack_from("<I", data, off + 4)[0]
        body = off + 8
        if cid == b"data":
            if fmt is None:
                raise ValueError(f"{path}: no 'fmt ' chunk before the 'data' chunk")
            if size == 0xFFFFFFFF or body + size > len(data):
                size = len(data) - body
            tag, channels, rate, bits = fmt
            frame = channels * bits // 8
            n_frames = size // frame
            kind = {(_WAV_PCM, 8): _lib.PCM_U8, (_WAV_PCM, 16): _lib.PCM_S16, (_WAV_PCM, 24): _lib.PCM_S24,
                    (_WAV_PCM, 32): _lib.PCM_S32, (_WAV_FLOAT, 32): _lib.PCM_F32, (_WAV_FLOAT, 64): _lib.PCM_F64}
            return data[body:body + n_frames * frame], rate, channels, kind[tag, bits], n_frames
        if cid == b"fmt ":
            if size < 16 or body + 16 > len(data):
                raise ValueError(f"{path}: 'fmt ' chunk of {size} bytes is too short")
            tag, channels, rate, _, _, bits = struct.unpack_from("<HHIIHH", data, body)
            if tag == _WAV_EXTENSIBLE:
                if size < 40 or body + 40 > len(data):
                    raise ValueError(f"{path}: EXTENSIBLE 'fmt ' chunk of {size} bytes is too short")
                tag = struct.unpack_from("<H", data, body + 24)[0]
            if tag not in (_WAV_PCM, _WAV_FLOAT):
                name = _WAV_COMPRESSED[tag] + ", compressed" if tag in _WAV_COMPRESSED else "unknown"
                raise ValueError(f"{path}: unsupported audio format tag 0x{tag:04x} ({name}): only PCM and IEEE "
                                 "float samples are read")
            if bits not in ((8, 16, 24, 32) if tag == _WAV_PCM else (32, 64)):
                raise ValueError(f"{path}: unsupported {'PCM' if tag == _WAV_PCM else 'IEEE float'} sample size of "
                                 f"{bits} bits")
            if channels == 0:
                raise ValueError(f"{path}: zero channels")
            if rate == 0:
                raise ValueError(f"{path}: zero sample rate")
            fmt = (tag, channels, rate, bits)
        off = body + size + (size & 1)
    raise ValueError(f"{path}: no 'data' chunk" if fmt is not None else f"{path}: no 'fmt ' chunk")


def resample_table(sr_in: int, sr_out: int):
    """-> (table, up, down, half): the filter of inference.resample, phase-major float32 [up, row_stride] (row p:
    the 2 half taps of the outputs with k mod up == p, taps ascending; row_stride = 2 half rounded up to 4 floats
    with zeros, so every row is 16-byte aligned).  The arithmetic is inference.resample's, in float64, rounded to
    float32 once.  Equal rates: (None, 1, 1, 0).  Cached per rate pair.  A pair whose table would exceed
    TABLE_MAX_FLOATS (192001 -> 16000, say: 16000 phases of 1622 taps) raises ValueError before anything is allocated."""
    key = sr_in, sr_out = int(sr_in), int(sr_out)
    if key in _RESAMPLE:
        return _RESAMPLE[key]
    num_zeros, rolloff, beta = KAISER_BEST
    if sr_in < 1 or sr_out < 1:
        raise ValueError(f"resample_table: sample rates must be positive (got {sr_in} -> {sr_out})")
    if sr_in == sr_out:
        res = (None, 1, 1, 0)
    else:
        g = math.gcd(sr_in, sr_out)
        up, down = sr_out // g, sr_in // g
        cutoff = rolloff * min(1.0, sr_out / sr_in)
        half = int(math.ceil(num_zeros / cutoff))
        row_stride = (2 * half + 3) // 4 * 4
        if up * row_stride > TABLE_MAX_FLOATS:
            raise ValueError(f"resample_table: {sr_in} Hz -> {sr_out} Hz needs {up} phases of {2 * half} taps, more "
                             f"than {TABLE_MAX_FLOATS} floats; resample the file to a standard rate first")
        taps = np.arange(-half + 1, half + 1)
        phases = np.arange(up) * down % up / up
        t = taps[None, :] - phases[:, None]
        win = np.i0(beta * np.sqrt(np.clip(1.0 - (t / (half + 1)) ** 2, 0.0, 1.0))) / np.i0(beta)
        filt = (cutoff * np.sinc(cutoff * t) * win).astype(np.float64)
        table = np.zeros((up, row_stride), np.float32)
        table[:, :2 * half] = filt.astype(np.float32)
        table.setflags(write=False)
        res = (table, up, down, half)
    _RESAMPLE[key] = res
    return res


def _device_table(sr_in: int, sr_out: int, device):
    """resample_table on ``device``: uploaded once per rate pair and device."""
    table, up, down, half = resample_table(sr_in, sr_out)
    if table is None:
        return None, up, down, half
    key = (int(sr_in), int(sr_out), str(device))
    if key not in _RESAMPLE_DEV:
        _RESAMPLE_DEV[key] = torch.from_numpy(table.copy()).to(device)
    return _RESAMPLE_DEV[key], up, down, half


def resampled_length(n_frames: int, sr_in: int, sr_out: int) -> int:
    """ceil(n_frames sr_out / sr_in), the length inference.resample gives, in integers."""
    g = math.gcd(sr_in, sr_out)
    return -(-n_frames * (sr_out // g) // (sr_in // g))


def load_audio(path: str, sr: int = 16000, device="cuda", out: torch.Tensor | None = None) -> torch.Tensor:
    """inference.load_wav on the device: float32 [n_out] mono at ``sr`` of a file read_wav reads.  One upload of
    the file's sample bytes and one launch (s2v_audio_load): the host does no arithmetic on the samples.  ``out``:
    a contiguous float32 device vector of resampled_length(n_frames, rate, sr) elements to write into."""
    raw, rate, channels, fmt, n_frames = read_wav(path)
    device = torch.device(device) if out is None else out.device
    if device.type != "cuda":
        raise _lib.S2VError("load_audio runs on the HIP device only")
    n_out = resampled_length(n_frames, rate, sr)
    if out is None:
        out = torch.empty(n_out, dtype=torch.float32, device=device)
    elif out.shape != (n_out,):
        raise ValueError(f"load_audio: out must hold {n_out} samples, got {tuple(out.shape)}")
    if n_frames == 0:
        return out
    table, up, down, half = _device_table(rate, sr, device)
    pcm = torch.frombuffer(raw, dtype=torch.uint8).to(device)
    ops.S2V.audio_load_(pcm, n_frames, channels, fmt, table, up, down, half, out)
    return out


def pcm16(path: str):
    """(interleaved PCM as int16 [frames, channels], rate) of a file read_wav reads, at its own rate and channel
    count: what mjpeg.wav_pcm16 gives for the integer formats (8 bit: (v - 128) << 8; 24 and 32 bit: the upper
    16 bits); float samples are clip(rint(x 32768), -32768, 32767)."""
    raw, rate, channels, fmt, n_frames = read_wav(path)
    if fmt == _lib.PCM_S16:
        pcm = np.frombuffer(raw, "<i2")
    elif fmt == _lib.PCM_U8:
        pcm = ((np.frombuffer(raw, np.uint8).astype(np.int16) - 128) << 8).astype("<i2")
    elif fmt == _lib.PCM_S24:
        b = np.frombuffer(raw, np.uint8).reshape(-1, 3)
        pcm = (b[:, 1].astype(np.uint16) | (b[:, 2].astype(np.uint16) << 8)).astype("<u2").view("<i2")
    elif fmt == _lib.PCM_S32:
        pcm = (np.frombuffer(raw, "<i4") >> 16).astype("<i2")
    else:
        x = np.frombuffer(raw, "<f4" if fmt == _lib.PCM_F32 else "<f8")
        pcm = np.clip(np.rint(x * 32768.0), -32768, 32767).astype("<i2")
    return np.ascontiguousarray(pcm.reshape(-1, channels)), rate
