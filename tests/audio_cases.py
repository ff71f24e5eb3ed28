"""The audio loader's contract (include/s2v.h, s2v_audio_load; s2v_amd.audio.load_audio) restated in float64 NumPy
without calling s2v_amd.audio, and writers of the RIFF/WAVE files its tests read.

    out[k] = sum_{t = -half+1 .. half} x[floor(k down / up) + t] * filt[k mod up][t + half - 1]

``filter64`` is the filter of inference.resample (librosa 0.9 'kaiser_best': 64 zero crossings, rolloff 0.9476,
Kaiser beta 14.77) in float64; ``reference`` evaluates any window of outputs directly, so a test of a long clip needs
only the outputs it looks at."""
import math
import struct

import numpy as np

NUM_ZEROS, ROLLOFF, BETA = 64, 0.9475937167399596, 14.769656459379492
FORMATS = ("u8", "s16", "s24", "s32", "f32", "f64")          # in the order of the S2V_PCM_* enum
TAG = {"u8": (1, 8), "s16": (1, 16), "s24": (1, 24), "s32": (1, 32), "f32": (3, 32), "f64": (3, 64)}
# KSDATAFORMAT_SUBTYPE_*: the format tag, then this tail
GUID_TAIL = bytes.fromhex("000000001000800000aa00389b71")


# ----------------------------------------------------------------------------- the operation
def ratio(sr_in, sr_out):
    g = math.gcd(sr_in, sr_out)
    return sr_out // g, sr_in // g                           # up, down


def host_length(n, sr_in, sr_out):
    """inference.resample's output length"""
    return n if sr_in == sr_out else int(math.ceil(n * sr_out / sr_in))


def filter64(sr_in, sr_out):
    """-> (filt float64 [up, 2 half], up, down, half)"""
    up, down = ratio(sr_in, sr_out)
    cutoff = ROLLOFF * min(1.0, sr_out / sr_in)
    half = int(math.ceil(NUM_ZEROS / cutoff))
    taps = np.arange(-half + 1, half + 1)
    phases = np.arange(up) * down % up / up
    t = taps[None, :] - phases[:, None]
    win = np.i0(BETA * np.sqrt(np.clip(1.0 - (t / (half + 1)) ** 2, 0.0, 1.0))) / np.i0(BETA)
    return cutoff * np.sinc(cutoff * t) * win, up, down, half


def reference(x, sr_in, sr_out, k0=0, k1=None):
    """Outputs k0 <= k < k1 of the operation over the mono clip ``x`` in float64 (x is zero outside itself)."""
    x = np.asarray(x, np.float64)
    if k1 is None:
        k1 = host_length(len(x), sr_in, sr_out)
    if sr_in == sr_out:
        return x[k0:k1].copy()
    filt, up, down, half = filter64(sr_in, sr_out)
    out = np.empty(k1 - k0, np.float64)
    for s in range(k0, k1, 4096):
        k = np.arange(s, min(k1, s + 4096), dtype=np.int64)
        idx = (k * down // up)[:, None] + np.arange(-half + 1, half + 1)[None, :]
        ok = (idx >= 0) & (idx < len(x))
        xs = np.where(ok, x[np.clip(idx, 0, max(len(x) - 1, 0))] if len(x) else 0.0, 0.0)
        out[s - k0:s - k0 + len(k)] = np.einsum("ij,ij->i", xs, filt[k % up])
    return out


def tolerance(table32, half, peak):
    """The fp32 bound of one output: gamma_m * max_p sum_t |table[p][t]| * max|x| with m = 2 half + 2 roundings:
    2 half fused multiply-adds, the table's own rounding to float32 and the input's / the stored result's."""
    m = 2 * half + 2
    u = 2.0 ** -24
    gamma = m * u / (1.0 - m * u)
    return gamma * float(np.abs(np.asarray(table32, np.float64)).sum(axis=1).max()) * float(peak)


def impulse_spacing(down, half):
    """The smallest spacing >= 2 half + 1 (no output reaches two impulses) that is coprime to ``down`` (the impulses
    then meet every phase)."""
    s = 2 * half + 1
    while math.gcd(s, down) != 1:
        s += 1
    return s


def impulse_response(table32, up, down, half, positions, values, n_out):
    """The output of a clip that is zero except for values[i] (+-1.0) at positions[i], no two closer than 2 half + 1:
    every output holds at most one product 1 * f, which fp32 gives exactly.  -> (float32 [n_out], reached bool
    [up, 2 half]: the (phase, tap) pairs the impulses touch)."""
    out = np.zeros(n_out, np.float32)
    reached = np.zeros((up, 2 * half), bool)
    for p, v in zip(positions, values):
        lo = max(0, -((-(p - half) * up) // down))           # first k with floor(k down / up) >= p - half
        hi = min(n_out, -((-(p + half) * up) // down))       # first k with floor(k down / up) >= p + half
        if hi <= lo:
            continue
        k = np.arange(lo, hi, dtype=np.int64)
        tap = p - k * down // up + half - 1
        assert tap.min() >= 0 and tap.max() < 2 * half
        out[k] = np.float32(v) * table32[k % up, tap]
        reached[k % up, tap] = True
    return out, reached


# ----------------------------------------------------------------------------- samples and files
def random_codes(fmt, n, channels, seed=0):
    """Full-range random integer codes [n, channels] (int64) with the extreme codes at the front."""
    bits = TAG[fmt][1]
    lo, hi = (0, 255) if fmt == "u8" else (-(1 << (bits - 1)), (1 << (bits - 1)) - 1)
    v = np.random.default_rng(seed).integers(lo, hi + 1, size=(n, channels), dtype=np.int64)
    flat = v.reshape(-1)
    ext = np.array([lo, hi, lo, lo, hi, hi, 0 if fmt != "u8" else 128, lo + 1, hi - 1], np.int64)
    flat[:min(len(ext), len(flat))] = ext[:len(flat)]
    return v


def encode(samples, fmt):
    """[n, channels] integer codes (u8 / s16 / s24 / s32) or floats (f32 / f64) -> interleaved little-endian bytes"""
    a = np.asarray(samples)
    if fmt == "u8":
        return a.astype(np.uint8).tobytes()
    if fmt == "s16":
        return a.astype("<i2").tobytes()
    if fmt == "s24":
        b = a.astype("<i4").reshape(-1).view(np.uint8).reshape(-1, 4)
        return np.ascontiguousarray(b[:, :3]).tobytes()
    if fmt == "s32":
        return a.astype("<i4").tobytes()
    return a.astype("<f4" if fmt == "f32" else "<f8").tobytes()


def decode(samples, fmt):
    """What the loader makes of those samples before the downmix: float32 [n, channels]"""
    a = np.asarray(samples)
    if fmt == "u8":
        return (a.astype(np.float32) - np.float32(128)) / np.float32(128)
    if fmt in ("s16", "s24", "s32"):
        return a.astype(np.int32).astype(np.float32) / np.float32(1 << (TAG[fmt][1] - 1))
    return a.astype(np.float32)


def chunk(cid, body):
    return cid + struct.pack("<I", len(body)) + body + (b"\0" if len(body) & 1 else b"")


def fmt_chunk(fmt, rate, channels, extensible=False, tag=None, bits=None):
    t, b = TAG[fmt] if fmt else (tag, bits)
    t = t if tag is None else tag
    b = b if bits is None else bits
    align = channels * b // 8
    if not extensible:
        return chunk(b"fmt ", struct.pack("<HHIIHH", t, channels, rate, rate * align, align, b))
    return chunk(b"fmt ", struct.pack("<HHIIHHHHI", 0xFFFE, channels, rate, rate * align, align, b, 22, b,
                                      (1 << channels) - 1) + struct.pack("<H", t) + GUID_TAIL)


def wav_bytes(data, fmt, rate, channels, extensible=False, before=(), after=(), data_size=None, tag=None, bits=None):
    """A RIFF/WAVE file: ``fmt `` (plain or EXTENSIBLE), the chunks ``before``, ``data``, the chunks ``after``.
    ``data_size``: the size the data chunk's header states (None: the true one)."""
    body = b"WAVE" + fmt_chunk(fmt, rate, channels, extensible, tag, bits) + b"".join(before)
    body += b"data" + struct.pack("<I", len(data) if data_size is None else data_size) + data
    if after or len(data) & 1 and data_size is None:
        body += (b"\0" if len(data) & 1 else b"") + b"".join(after)
    return b"RIFF" + struct.pack("<I", len(body) & 0xFFFFFFFF) + body


def write(path, samples, fmt, rate, **kw):
    """samples [n, channels] -> the file at ``path``; -> str(path)"""
    a = np.asarray(samples)
    with open(path, "wb") as f:
        f.write(wav_bytes(encode(a, fmt), fmt, rate, a.shape[1], **kw))
    return str(path)
