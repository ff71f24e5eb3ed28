"""Motion-JPEG output: the device JPEG encoder (csrc/jpeg.hip, s2v_jpeg_encode) and a RIFF AVI 1.0 writer
that carries the input audio — the counterpart of the reference's cv2.VideoWriter + ffmpeg mux
(inference.py:246-249, :325-336).

The stream contract (include/s2v.h) is all integer arithmetic: baseline JFIF, YCbCr 4:2:0, the
T.81 Annex K.3 Huffman tables, the Annex K.1 / K.2 quantisation tables scaled by the IJG rule, one restart
interval per MCU row.  ``jfif_header`` writes everything up to the entropy-coded data; the kernels write the
rest.  There is no decoder here and no other container: a user with ffmpeg transcodes the AVI.
"""
from __future__ import annotations

import struct
import wave
from fractions import Fraction

import numpy as np

# T.81 Annex K.1 (luminance) and K.2 (chrominance) quantisation tables, in zigzag order (a DQT segment's order)
K1_LUMA_ZIGZAG = (
    16, 11, 12, 14, 12, 10, 16, 14, 13, 14, 18, 17, 16, 19, 24, 40, 26, 24, 22, 22, 24, 49, 35, 37, 29, 40, 58, 51,
    61, 60, 57, 51, 56, 55, 64, 72, 92, 78, 64, 68, 87, 69, 55, 56, 80, 109, 81, 87, 95, 98, 103, 104, 103, 62, 77,
    113, 121, 112, 100, 120, 92, 101, 103, 99)
K2_CHROMA_ZIGZAG = (
    17, 18, 18, 24, 21, 24, 47, 26, 26, 47, 99, 66, 56, 66, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99,
    99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99,
    99, 99, 99, 99, 99, 99, 99, 99)

# T.81 Annex K.3 typical Huffman tables: (Tc << 4 | Th, BITS[16], HUFFVAL), in the header's order
K3_HUFFMAN = (
    (0x00, bytes.fromhex("00010501010101010100000000000000"), bytes(range(12))),
    (0x10, bytes.fromhex("0002010303020403050504040000017d"), bytes.fromhex(
        "01020300041105122131410613516107227114328191a1082342b1c11552d1f02433627282090a161718191a25262728292a"
        "3435363738393a434445464748494a535455565758595a636465666768696a737475767778797a"
        "838485868788898a92939495969798999aa2a3a4a5a6a7a8a9aab2b3b4b5b6b7b8b9ba"
        "c2c3c4c5c6c7c8c9cad2d3d4d5d6d7d8d9dae1e2e3e4e5e6e7e8e9eaf1f2f3f4f5f6f7f8f9fa")),
    (0x01, bytes.fromhex("00030101010101010101010000000000"), bytes(range(12))),
    (0x11, bytes.fromhex("00020102040403040705040400010277"), bytes.fromhex(
        "000102031104052131061241510761711322328108144291a1b1c109233352f0156272d10a162434e125f11718191a262728"
        "292a35363738393a434445464748494a535455565758595a636465666768696a737475767778797a"
        "82838485868788898a92939495969798999aa2a3a4a5a6a7a8a9aab2b3b4b5b6b7b8b9ba"
        "c2c3c4c5c6c7c8c9cad2d3d4d5d6d7d8d9dae2e3e4e5e6e7e8e9eaf2f3f4f5f6f7f8f9fa")),
)

AVI_MAX_BYTES = (1 << 31) - 1            # RIFF AVI 1.0 without OpenDML: one RIFF chunk below 2 GiB


def quant_tables(quality: int) -> np.ndarray:
    """uint16 [2, 64] (luma, chroma) in zigzag order: Annex K scaled by the IJG rule, entries 1..255."""
    q = int(quality)
    if not 1 <= q <= 100:
        raise ValueError(f"jpeg quality {quality}: 1 to 100")
    s = 5000 // q if q < 50 else 200 - 2 * q
    base = np.array([K1_LUMA_ZIGZAG, K2_CHROMA_ZIGZAG], np.int64)
    return np.clip((base * s + 50) // 100, 1, 255).astype(np.uint16)


def _segment(marker: int, body: bytes) -> bytes:
    return struct.pack(">BBH", 0xFF, marker, len(body) + 2) + body


def jfif_header(h: int, w: int, quality: int) -> bytes:
    """Everything before the entropy-coded data: SOI, APP0, DQT x2, SOF0, DHT x4, DRI, SOS."""
    if not (0 < h <= 65535 and 0 < w <= 65535):
        raise ValueError(f"jpeg frame size {h}x{w}: 1 to 65535")
    qt = quant_tables(quality)
    out = [b"\xff\xd8", _segment(0xE0, b"JFIF\0" + struct.pack(">BBBHHBB", 1, 1, 0, 1, 1, 0, 0))]
    for i in range(2):
        out.append(_segment(0xDB, bytes([i]) + bytes(qt[i].astype(np.uint8).tolist())))
    out.append(_segment(0xC0, struct.pack(">BHHB", 8, h, w, 3) + bytes([1, 0x22, 0, 2, 0x11, 1, 3, 0x11, 1])))
    for tc_th, bits, vals in K3_HUFFMAN:
        out.append(_segment(0xC4, bytes([tc_th]) + bits + vals))
    out.append(_segment(0xDD, struct.pack(">H", (w + 15) // 16)))
    out.append(_segment(0xDA, bytes([3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0])))
    return b"".join(out)


class JpegEncoder:
    """Baseline JPEG of uint8 [n, h, w, 3] device frames on the device, one launch sequence per batch."""

    def __init__(self, h: int, w: int, quality: int = 95, order: str = "bgr", device="cuda"):
        import torch

        from . import _lib
        if order not in ("bgr", "rgb"):
            raise ValueError(f"channel order {order!r}: 'bgr' or 'rgb'")
        self.h, self.w, self.quality, self.order = int(h), int(w), int(quality), order
        self.device = torch.device(device)
        self.header = jfif_header(self.h, self.w, self.quality)
        self.lib = _lib.load()
        self.worst = int(self.lib.s2v_jpeg_worst_bytes(self.h, self.w))
        self.capacity = len(self.header) + max(65536, self.h * self.w * 3 // 2)
        self._header = torch.frombuffer(bytearray(self.header), dtype=torch.uint8).to(self.device)
        self._qt = torch.from_numpy(quant_tables(self.quality).astype(np.int16)).to(self.device)   # bits of uint16
        self._ws = None
        self._ws_n = 0

    def _workspace(self, n: int):
        import torch
        if self._ws is None or self._ws_n < n:
            nbytes = int(self.lib.s2v_jpeg_ws_bytes(n, self.h, self.w))
            self._ws = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
            self._ws_n = n
        return self._ws

    def encode(self, frames, capacity: int | None = None, out=None):
        """frames uint8 [n, h, w, 3] on the device (a view with channel stride 1 and pixel stride 3 is taken as
        it lies) -> (out uint8 [n, capacity], sizes int32 [n], status int32 [n]), all on the device: frame b's
        file is out[b, :sizes[b]] when status[b] == 0; status[b] == 1: it needs sizes[b] > capacity bytes."""
        import torch

        from ._lib import check
        if frames.dtype != torch.uint8 or frames.dim() != 4 or tuple(frames.shape[1:]) != (self.h, self.w, 3):
            raise ValueError(f"frames {tuple(frames.shape)} {frames.dtype}: uint8 [n, {self.h}, {self.w}, 3]")
        if frames.device.type != self.device.type:
            raise ValueError(f"frames on {frames.device}: the encoder is on {self.device}")
        n = frames.shape[0]
        if n == 0:
            raise ValueError("no frames")
        sn, sy, sx, sc = frames.stride()
        if sc != 1 or sx != 3 or sy < 3 * self.w or (n > 1 and sn < 0):
            frames = frames.contiguous()
            sn, sy, sx, sc = frames.stride()
        capacity = int(capacity or self.capacity)
        if out is None:
            out = torch.empty((n, capacity), dtype=torch.uint8, device=self.device)
        elif out.dtype != torch.uint8 or tuple(out.shape) != (n, capacity) or not out.is_contiguous():
            raise ValueError(f"out {tuple(out.shape)}: contiguous uint8 [{n}, {capacity}]")
        sizes = torch.empty((n,), dtype=torch.int32, device=self.device)
        status = torch.empty((n,), dtype=torch.int32, device=self.device)
        ws = self._workspace(n)
        check(self.lib.s2v_jpeg_encode(frames.data_ptr(), n, self.h, self.w, sy, sn, 1 if self.order == "bgr" else 0,
                                       self._header.data_ptr(), len(self.header), self._qt.data_ptr(),
                                       out.data_ptr(), capacity, sizes.data_ptr(), status.data_ptr(), ws.data_ptr(),
                                       ws.numel(), torch.cuda.current_stream(self.device).cuda_stream),
              "s2v_jpeg_encode")
        return out, sizes, status

    def encode_to_host(self, frames) -> list:
        """-> one ``bytes`` JPEG file per frame.  One device -> host copy of the sizes, one of the used bytes; a
        frame that does not fit the default capacity is encoded again alone with the worst-case capacity."""
        import torch
        out, sizes, status = self.encode(frames)
        meta = torch.stack([sizes, status]).cpu().numpy()
        sz, st = meta[0].tolist(), meta[1].tolist()
        used = max([s for s, t in zip(sz, st) if t == 0], default=0)
        host = out[:, :used].cpu().numpy() if used else None
        files = []
        for b, (s, t) in enumerate(zip(sz, st)):
            if t == 0:
                files.append(host[b, :s].tobytes())
                continue
            o1, s1, t1 = self.encode(frames[b:b + 1], capacity=len(self.header) + self.worst)
            s1, t1 = int(s1.item()), int(t1.item())
            if t1 != 0:
                raise RuntimeError(f"jpeg frame {b}: {s1} bytes exceed the worst-case bound")
            files.append(o1[0, :s1].cpu().numpy().tobytes())
        return files


def wav_pcm16(path: str):
    """(interleaved PCM as int16 [frames, channels], rate) of a PCM .wav at its own rate and channel count;
    8-, 24- and 32-bit files are converted to 16 bits."""
    with wave.open(path, "rb") as w:
        ch, width, rate, n = w.getnchannels(), w.getsampwidth(), w.getframerate(), w.getnframes()
        raw = w.readframes(n)
    if width == 2:
        pcm = np.frombuffer(raw, "<i2")
    elif width == 1:
        pcm = ((np.frombuffer(raw, np.uint8).astype(np.int16) - 128) << 8).astype("<i2")
    elif width == 3:
        b = np.frombuffer(raw, np.uint8).reshape(-1, 3)
        pcm = (b[:, 1].astype(np.uint16) | (b[:, 2].astype(np.uint16) << 8)).astype("<u2").view("<i2")
    elif width == 4:
        pcm = (np.frombuffer(raw, "<i4") >> 16).astype("<i2")
    else:
        raise ValueError(f"unsupported PCM sample width {width}")
    return np.ascontiguousarray(pcm.reshape(-1, ch)), rate


def _chunk(fourcc: bytes, body: bytes) -> bytes:
    return fourcc + struct.pack("<I", len(body)) + body + (b"\0" if len(body) & 1 else b"")


class AviWriter:
    """RIFF AVI 1.0 with one MJPG video stream and, with ``audio`` = (int16 [frames, channels], rate), one
    16-bit PCM stream cut to the video's duration: ``movi`` holds one 00dc chunk per frame, each followed by
    that frame's 01wb audio chunk; ``idx1`` closes the file.  The headers are written by close()."""

    def __init__(self, path, w: int, h: int, fps, audio=None, max_bytes: int = AVI_MAX_BYTES):
        self.path, self.w, self.h = str(path), int(w), int(h)
        fr = Fraction(fps).limit_denominator(100000)
        if fr <= 0:
            raise ValueError(f"fps {fps}")
        self.rate, self.scale = fr.numerator, fr.denominator
        self.max_bytes = min(int(max_bytes), AVI_MAX_BYTES)
        self.pcm = self.audio_rate = None
        self.channels = 0
        if audio is not None:
            pcm, rate = audio
            pcm = np.asarray(pcm)
            if pcm.dtype != np.int16 or pcm.ndim != 2 or pcm.shape[1] < 1 or int(rate) <= 0:
                raise ValueError("audio: (int16 [frames, channels], rate)")
            self.pcm, self.audio_rate, self.channels = np.ascontiguousarray(pcm.astype("<i2")), int(rate), pcm.shape[1]
        self.frames = 0
        self.audio_frames = 0              # sample frames written so far
        self.max_video = self.max_audio = 0
        self.index = []                    # (fourcc, offset from the 'movi' fourcc, size)
        self.movi_bytes = 4                # the 'movi' fourcc itself
        self._hdr_bytes = len(self._headers())
        self._f = open(self.path, "wb")
        self._f.write(bytes(self._hdr_bytes))
        self.closed = False

    def _audio_until(self, frames: int) -> int:
        """sample frames of audio that belong to the first ``frames`` video frames"""
        return min(len(self.pcm), frames * self.audio_rate * self.scale // self.rate)

    def _file_bytes(self, extra: int = 0, entries: int = 0) -> int:
        return self._hdr_bytes + self.movi_bytes - 4 + extra + 8 + 16 * (len(self.index) + entries)

    def _put(self, fourcc: bytes, body: bytes):
        ck = _chunk(fourcc, body)
        self.index.append((fourcc, self.movi_bytes, len(body)))
        self._f.write(ck)
        self.movi_bytes += len(ck)

    def write(self, jpeg_bytes: bytes):
        if self.closed:
            raise ValueError("AviWriter is closed")
        jpeg_bytes = bytes(jpeg_bytes)
        a0 = a1 = 0
        if self.pcm is not None:
            a0, a1 = self.audio_frames, self._audio_until(self.frames + 1)
        abytes = (a1 - a0) * 2 * self.channels
        extra = 8 + len(jpeg_bytes) + (len(jpeg_bytes) & 1) + ((8 + abytes) if a1 > a0 else 0)
        if self._file_bytes(extra, 2 if a1 > a0 else 1) > self.max_bytes:
            raise ValueError(f"{self.path}: frame {self.frames} would take the file past {self.max_bytes} bytes "
                             "(RIFF AVI 1.0 ends below 2 GiB; OpenDML is not written)")
        self._put(b"00dc", jpeg_bytes)
        self.max_video = max(self.max_video, len(jpeg_bytes))
        self.frames += 1
        if a1 > a0:
            self._put(b"01wb", self.pcm[a0:a1].tobytes())
            self.max_audio = max(self.max_audio, abytes)
            self.audio_frames = a1

    def _headers(self) -> bytes:
        """RIFF header, hdrl and the LIST header of movi up to its fourcc, for the counts so far"""
        has_audio = self.pcm is not None
        usec = round(1e6 * self.scale / self.rate)
        per_sec = 0 if not self.frames else (self.movi_bytes * self.rate) // (self.scale * self.frames)
        avih = struct.pack("<14I", usec, per_sec, 0, 0x10 | 0x100, self.frames, 0, 2 if has_audio else 1,
                           max(self.max_video, self.max_audio), self.w, self.h, 0, 0, 0, 0)
        strh_v = struct.pack("<4s4sIHHIIIIIIII4H", b"vids", b"MJPG", 0, 0, 0, 0, self.scale, self.rate, 0, self.frames,
                             self.max_video, 0xFFFFFFFF, 0, 0, 0, self.w, self.h)
        strf_v = struct.pack("<IiiHH4sIiiII", 40, self.w, self.h, 1, 24, b"MJPG", self.w * self.h * 3, 0, 0, 0, 0)
        strl = [_chunk(b"LIST", b"strl" + _chunk(b"strh", strh_v) + _chunk(b"strf", strf_v))]
        if has_audio:
            align = 2 * self.channels
            strh_a = struct.pack("<4s4sIHHIIIIIIII4H", b"auds", b"\0\0\0\0", 0, 0, 0, 0, 1, self.audio_rate, 0,
                                 self.audio_frames, self.max_audio, 0xFFFFFFFF, align, 0, 0, 0, 0)
            strf_a = struct.pack("<HHIIHHH", 1, self.channels, self.audio_rate, self.audio_rate * align, align, 16, 0)
            strl.append(_chunk(b"LIST", b"strl" + _chunk(b"strh", strh_a) + _chunk(b"strf", strf_a)))
        hdrl = _chunk(b"LIST", b"hdrl" + _chunk(b"avih", avih) + b"".join(strl))
        riff_size = 4 + len(hdrl) + 8 + self.movi_bytes + 8 + 16 * len(self.index)
        return (b"RIFF" + struct.pack("<I", riff_size) + b"AVI " + hdrl + b"LIST" + struct.pack("<I", self.movi_bytes)
                + b"movi")

    def close(self):
        if self.closed:
            return
        self.closed = True
        idx = b"".join(struct.pack("<4sIII", cc, 0x10, off, size) for cc, off, size in self.index)
        self._f.write(b"idx1" + struct.pack("<I", len(idx)) + idx)
        self._f.seek(0)
        hdr = self._headers()
        assert len(hdr) == self._hdr_bytes
        self._f.write(hdr)
        self._f.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
