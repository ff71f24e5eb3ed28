"""Motion-JPEG in and out: the device JPEG encoder (csrc/jpeg.hip, s2v_jpeg_encode) and decoder
(csrc/jpeg_dec.hip, s2v_jpeg_decode), and a RIFF AVI 1.0 writer and reader that carry the audio -- the counterpart of
the reference's cv2.VideoCapture / cv2.VideoWriter + ffmpeg mux (inference.py:58-64, :246-249, :325-336).

The encoder's stream contract (include/s2v.h) is all integer arithmetic: baseline JFIF, YCbCr 4:2:0,
the T.81 Annex K.3 Huffman tables, the Annex K.1 / K.2 quantisation tables scaled by the IJG rule, one restart
interval per MCU row.  ``jfif_header`` writes everything up to the entropy-coded data; the kernels write the rest.

The decoder takes any baseline stream ``parse_jpeg`` accepts -- SOF0, 8 bit, YCbCr at 4:4:4, 4:2:2
or 4:2:0, one interleaved scan, any tables, any restart interval -- and gives libjpeg's pixels bit for bit.  Its unit
of parallel work is the restart interval: a stream without restart markers (Pillow's and ffmpeg's default) is decoded
by one lane per frame, correct and slow, unless the opt-in ``split="sync"`` (s2v_jpeg_decode_sync) decodes inside the
interval in parallel.  ``ffmpeg -i in.mp4 -c:v mjpeg -q:v 2 out.avi`` makes a file ``AviReader`` reads.  There is no
MP4 and no other codec: a user with ffmpeg transcodes.
"""
from __future__ import annotations

import os
import struct
import wave
from dataclasses import dataclass
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


HUFF_SPEC_BYTES = 16 + 256               # a table as the decoder takes it: BITS[16], HUFFVAL[256]
SAMPLINGS = {(1, 1): 0, (2, 1): 1, (2, 2): 2}      # luma (h, v) sampling -> Pillow's subsampling number
_SOF_NAMES = {0xC1: "extended sequential", 0xC2: "progressive", 0xC3: "lossless", 0xC5: "differential sequential",
              0xC6: "differential progressive", 0xC7: "differential lossless", 0xC9: "arithmetic-coded sequential",
              0xCA: "arithmetic-coded progressive", 0xCB: "arithmetic-coded lossless", 0xCD: "arithmetic-coded",
              0xCE: "arithmetic-coded", 0xCF: "arithmetic-coded"}


@dataclass
class JpegInfo:
    """What the headers of one baseline JPEG file say (parse_jpeg)."""
    h: int
    w: int
    sampling: int                  # 0 = 4:4:4, 1 = 4:2:2, 2 = 4:2:0
    qtables: np.ndarray            # uint16 [3, 64]: component c's table in zigzag order
    huffman: bytes                 # six tables, (DC, AC) of components 0, 1, 2, each BITS[16] + HUFFVAL[256]
    restart_interval: int          # MCUs per restart interval, 0: none
    scan: tuple                    # (start, end) of the entropy-coded segment in the file, markers after it excluded
    mcols: int
    mrows: int

    @property
    def mcus(self) -> int:
        return self.mcols * self.mrows


def _huff_spec(bits: bytes, vals: bytes, what: str) -> bytes:
    if len(vals) != sum(bits) or len(vals) > 256:
        raise ValueError(f"{what}: {sum(bits)} codes for {len(vals)} values")
    code = 0
    for length in range(1, 17):
        code = (code + bits[length - 1]) << 1
        if code > 2 << length:
            raise ValueError(f"{what}: more codes of {length} bits than there are")
    return bytes(bits) + bytes(vals) + bytes(256 - len(vals))


def parse_jpeg(data) -> JpegInfo:
    """The headers of a baseline JPEG file: SOF0, 8 bit, three components (YCbCr) with luma sampling 2x2, 2x1 or 1x1
    and chroma 1x1, 8-bit DQT, one interleaved scan, any DRI.  A file without DHT gets the Annex K.3 tables (the AVI
    MJPG convention).  Everything else raises ValueError naming what it found."""
    data = bytes(data)
    if data[:2] != b"\xff\xd8":
        raise ValueError("not a JPEG file: no SOI marker")
    qt, huff, frame, dri, adobe = {}, {}, None, 0, None
    i = 2
    while True:
        if i + 4 > len(data):
            raise ValueError("JPEG headers end before a scan (SOS)")
        if data[i] != 0xFF:
            raise ValueError(f"byte {i}: 0x{data[i]:02x} where a marker should be")
        m = data[i + 1]
        if m == 0xFF:                                      # fill byte
            i += 1
            continue
        if m == 0x01 or 0xD0 <= m <= 0xD8:
            i += 2
            continue
        if m == 0xD9:
            raise ValueError("JPEG file ends (EOI) before a scan")
        (length,) = struct.unpack(">H", data[i + 2:i + 4])
        body = data[i + 4:i + 2 + length]
        if length < 2 or len(body) != length - 2:
            raise ValueError(f"marker 0x{m:02x} at byte {i}: segment of {length} bytes runs past the file")
        i += 2 + length
        if m in _SOF_NAMES:
            raise ValueError(f"{_SOF_NAMES[m]} JPEG (SOF{m - 0xC0}): only baseline (SOF0) is decoded")
        if m == 0xC0:
            if frame is not None:
                raise ValueError("two SOF0 segments")
            prec, h, w, nc = struct.unpack(">BHHB", body[:6])
            if prec != 8:
                raise ValueError(f"{prec}-bit JPEG: only 8-bit samples are decoded")
            if nc != 3:
                kind = {1: "greyscale", 4: "CMYK / YCCK"}.get(nc, f"{nc}-component")
                raise ValueError(f"{kind} JPEG ({nc} component{'s' * (nc != 1)}): only YCbCr is decoded")
            if h == 0 or w == 0 or len(body) != 6 + 3 * nc:
                raise ValueError(f"SOF0: frame size {h}x{w}, {len(body)} bytes")
            frame = (h, w, [(body[6 + 3 * c], body[7 + 3 * c] >> 4, body[7 + 3 * c] & 15, body[8 + 3 * c])
                            for c in range(3)])
        elif m == 0xDB:
            k = 0
            while k < len(body):
                pq, tq = body[k] >> 4, body[k] & 15
                if pq != 0:
                    raise ValueError(f"16-bit DQT (table {tq}): only 8-bit quantisation tables are decoded")
                if tq > 3 or k + 65 > len(body):
                    raise ValueError(f"DQT: table {tq}, segment too short")
                qt[tq] = np.frombuffer(body[k + 1:k + 65], np.uint8).astype(np.uint16)
                k += 65
        elif m == 0xC4:
            k = 0
            while k < len(body):
                tc_th = body[k]
                bits = body[k + 1:k + 17]
                if (tc_th >> 4) > 1 or (tc_th & 15) > 3 or len(bits) != 16 or k + 17 + sum(bits) > len(body):
                    raise ValueError(f"DHT: table 0x{tc_th:02x}, segment too short")
                huff[tc_th] = _huff_spec(bits, body[k + 17:k + 17 + sum(bits)], f"DHT 0x{tc_th:02x}")
                k += 17 + sum(bits)
        elif m == 0xDD:
            (dri,) = struct.unpack(">H", body[:2])
        elif m == 0xEE and body[:5] == b"Adobe" and len(body) >= 12:
            adobe = body[11]
        elif m == 0xDA:
            break
    if frame is None:
        raise ValueError("SOS before SOF0")
    h, w, comps = frame
    if adobe == 0:
        raise ValueError("RGB JPEG (Adobe transform 0): only YCbCr is decoded")
    ns = body[0]
    if ns != 3 or len(body) != 1 + 2 * ns + 3:
        raise ValueError(f"a scan of {ns} component{'s' * (ns != 1)}: multiple scans are not decoded, only one "
                         "interleaved scan of all three")
    if tuple(body[1 + 2 * ns:]) != (0, 63, 0):
        raise ValueError(f"scan parameters {tuple(body[1 + 2 * ns:])}: a baseline scan has (0, 63, 0)")
    if [body[1 + 2 * c] for c in range(3)] != [c[0] for c in comps]:
        raise ValueError("scan components are not the frame's, in its order")
    if (comps[1][1], comps[1][2], comps[2][1], comps[2][2]) != (1, 1, 1, 1) or (comps[0][1], comps[0][2]) not in SAMPLINGS:
        raise ValueError("sampling factors " + ", ".join(f"{c[1]}x{c[2]}" for c in comps)
                         + ": luma 2x2, 2x1 or 1x1 with chroma 1x1 is decoded")
    if not huff:
        huff = {tc_th: _huff_spec(bits, vals, "Annex K") for tc_th, bits, vals in K3_HUFFMAN}
    tables = []
    for c in range(3):
        td, ta = body[2 + 2 * c] >> 4, body[2 + 2 * c] & 15
        for key, what in ((td, "DC"), (0x10 | ta, "AC")):
            if key not in huff:
                raise ValueError(f"component {c}: {what} Huffman table {key & 15} is not defined")
            tables.append(huff[key])
        if comps[c][3] not in qt:
            raise ValueError(f"component {c}: quantisation table {comps[c][3]} is not defined")
    hs, vs = comps[0][1], comps[0][2]
    seg = np.frombuffer(data, np.uint8, offset=i)
    ff = np.nonzero(seg[:-1] == 0xFF)[0]
    nxt = seg[ff + 1]
    ends = ff[(nxt != 0) & ((nxt < 0xD0) | (nxt > 0xD7)) & (nxt != 0xFF)]
    end = i + (int(ends[0]) if len(ends) else len(seg))
    if len(ends) and data[end + 1] in (0xDA, 0xC4, 0xDB, 0xDD, 0xDC):
        raise ValueError(f"marker 0x{data[end + 1]:02x} after the first scan: multiple scans are not decoded")
    return JpegInfo(h, w, SAMPLINGS[(hs, vs)], np.stack([qt[c[3]] for c in comps]), b"".join(tables), dri, (i, end),
                    -(-w // (8 * hs)), -(-h // (8 * vs)))


def restart_intervals(data, info: JpegInfo) -> np.ndarray:
    """int32 [k, 4]: (byte offset in the file, byte length, first MCU, MCU count) of the restart intervals of the
    entropy-coded segment, the RSTm markers excluded.  ValueError unless there are exactly ceil(MCUs / interval) of
    them and the markers count 0..7 round and round."""
    start, end = info.scan
    seg = np.frombuffer(bytes(data), np.uint8)[start:end]
    ff = np.nonzero(seg[:-1] == 0xFF)[0] if len(seg) else np.zeros(0, np.int64)
    nxt = seg[ff + 1]
    at = ff[(nxt >= 0xD0) & (nxt <= 0xD7)]
    ri = info.restart_interval or info.mcus
    count = -(-info.mcus // ri)
    if len(at) != count - 1:
        raise ValueError(f"{len(at) + 1} restart intervals where {info.mcus} MCUs in intervals of {ri} make {count}")
    if not np.array_equal(seg[at + 1] - 0xD0, np.arange(count - 1) % 8):
        raise ValueError("restart markers out of sequence")
    begin = np.concatenate([[0], at + 2])
    stop = np.concatenate([at, [len(seg)]])
    first = np.arange(count) * ri
    return np.stack([begin + start, stop - begin, first, np.minimum(ri, info.mcus - first)], axis=1).astype(np.int32)


def _align16(n: int) -> int:
    return (n + 15) & ~15


def pack_streams(files, h: int, w: int, sampling: int):
    """The one host buffer a batch uploads and where its parts lie: (uint8 array, offsets dict, counts dict).
    Parts, each 16-byte aligned: intervals int32 [k, 5], frame_first int32 [n + 1], set_index int32 [n], qtables
    uint16 [n, 3, 64], huff_sets uint8 [s, 6, 272], then the files end to end."""
    files = [bytes(f) for f in files]
    if not files:
        raise ValueError("no files")
    rows, first, sets, set_index, qts, base = [], [0], {}, [], [], 0
    for b, f in enumerate(files):
        info = parse_jpeg(f)
        if (info.h, info.w, info.sampling) != (h, w, sampling):
            raise ValueError(f"file {b}: {info.h}x{info.w} sampling {info.sampling}; the decoder is for "
                             f"{h}x{w} sampling {sampling}")
        iv = restart_intervals(f, info)
        t = np.empty((len(iv), 5), np.int32)
        t[:, 0], t[:, 1], t[:, 2], t[:, 3:] = iv[:, 0] + base, iv[:, 1], b, iv[:, 2:]
        rows.append(t)
        first.append(first[-1] + len(iv))
        set_index.append(sets.setdefault(info.huffman, len(sets)))
        qts.append(info.qtables)
        base += len(f)
    if base >= 1 << 31:
        raise ValueError(f"{base} bytes of streams in one batch: below 2 GiB")
    parts = {"intervals": np.concatenate(rows), "frame_first": np.array(first, np.int32),
             "set_index": np.array(set_index, np.int32), "qtables": np.stack(qts).astype(np.uint16),
             "huff_sets": np.frombuffer(b"".join(sets), np.uint8), "data": np.frombuffer(b"".join(files), np.uint8)}
    offs, total = {}, 0
    for k, v in parts.items():
        offs[k] = total
        total = _align16(total + v.nbytes)
    buf = np.zeros(total, np.uint8)
    for k, v in parts.items():
        buf[offs[k]:offs[k] + v.nbytes] = np.ascontiguousarray(v).view(np.uint8).reshape(-1)
    counts = {"n": len(files), "intervals": int(first[-1]), "max_per_frame": int(np.diff(first).max()),
              "sets": len(sets), "data_bytes": base, "max_interval_bytes": int(parts["intervals"][:, 1].max())}
    return buf, offs, counts


JPEG_DECODE_ENV = "S2V_JPEG_DECODE"
JPEG_DECODE_MODES = ("wave", "lane", "sync", "auto")       # the entropy stage's split (JpegDecoder)
# Set from profiles/mjpeg_sync_micro.txt (tools/mjpeg_decode_micro.py --sync on an MI355X, 16 frames).
# SYNC_SUB_BYTES: of the sweep 64 .. 2048, 256 is the fastest on Pillow's 700x700 streams and within a quarter of
# the fastest (1024) at 1400x1400.  SYNC_AUTO_BYTES: "auto" takes sync when the batch's
# longest interval has more bytes than this.  In the crossover rows sync passes wave between 2.3 and 4.7 KB an interval
# and is 4 times faster at 17 KB; the project's own streams at 1400x1400 have intervals of 10 KB, 88 a frame, where
# sync at 256 bytes is no faster than wave: the threshold lies above them.
SYNC_SUB_BYTES = 256
SYNC_AUTO_BYTES = 16384


def jpeg_decode_mode(mode="wave") -> str:
    """A ``jpeg_decode=`` / ``split=`` name: one of JPEG_DECODE_MODES (0 and 1 are "wave" and "lane"); None reads
    S2V_JPEG_DECODE (unset or empty: "wave").  Anything else raises ValueError."""
    source = "jpeg_decode="
    if mode is None:
        mode, source = os.environ.get(JPEG_DECODE_ENV) or "wave", JPEG_DECODE_ENV + "="
    if mode in (0, 1) and not isinstance(mode, bool):
        mode = JPEG_DECODE_MODES[mode]
    if mode not in JPEG_DECODE_MODES:
        raise ValueError(f"{source}{mode!r}: {JPEG_DECODE_ENV} / jpeg_decode= takes one of "
                         f"{', '.join(JPEG_DECODE_MODES)}")
    return mode


class JpegDecoder:
    """Baseline JPEG files of one size and sampling -> uint8 [n, h, w, 3] device frames, one launch sequence and
    one host -> device copy per batch.  ``split``, the entropy stage: 0 / "wave" one wave per restart interval, 1 /
    "lane" one lane, "sync" one lane per ``sub_bytes`` (a multiple of 4 from 4 to 4096; None: SYNC_SUB_BYTES) of every
    interval (s2v_jpeg_decode_sync: for streams without restart markers), "auto" sync when the batch's longest
    interval exceeds SYNC_AUTO_BYTES, else wave.  Any other ``split`` (2, say) raises ValueError here, no longer in
    s2v_jpeg_decode at the first batch.  ``picked``: the split the last batch ran with."""

    def __init__(self, h: int, w: int, sampling: int = 2, order: str = "bgr", device="cuda", split=0,
                 sub_bytes: int | None = None):
        import torch

        from . import _lib
        if order not in ("bgr", "rgb"):
            raise ValueError(f"channel order {order!r}: 'bgr' or 'rgb'")
        if sampling not in (0, 1, 2):
            raise ValueError(f"sampling {sampling!r}: 0 (4:4:4), 1 (4:2:2) or 2 (4:2:0)")
        self.mode = jpeg_decode_mode(split)
        self.split = split if isinstance(split, str) else int(split)
        self.sub_bytes = SYNC_SUB_BYTES if sub_bytes is None else int(sub_bytes)
        if not (4 <= self.sub_bytes <= 4096 and self.sub_bytes % 4 == 0):
            raise ValueError(f"sub_bytes {sub_bytes!r}: a multiple of 4 from 4 to 4096")
        self.picked = None
        self.h, self.w, self.sampling, self.order = int(h), int(w), int(sampling), order
        self.device = torch.device(device)
        self.lib = _lib.load()
        self._ws = None
        self._ws_n = 0

    @classmethod
    def for_file(cls, data, **kw):
        info = parse_jpeg(data)
        return cls(info.h, info.w, info.sampling, **kw)

    def _workspace(self, n: int, nbytes: int = 0):
        import torch
        nbytes = nbytes or int(self.lib.s2v_jpeg_decode_ws_bytes(n, self.h, self.w, self.sampling))
        if self._ws is None or self._ws_n < n or self._ws.numel() < nbytes:
            self._ws = torch.empty(max(nbytes, 0 if self._ws is None else self._ws.numel()), dtype=torch.uint8,
                                   device=self.device)
            self._ws_n = max(n, self._ws_n)
        return self._ws

    def decode(self, files, out=None):
        """files: one ``bytes`` JPEG file per frame -> (frames uint8 [n, h, w, 3] on the device, status int32 [n] on
        the device).  ``out``: a uint8 [n, h, w, 3] device tensor or view with channel stride 1 and pixel stride 3
        to decode into.  status[b] != 0 (s2v_jpeg_decode): frame b's stream is damaged, its pixels are unspecified."""
        import torch
        buf, offs, cnt = pack_streams(files, self.h, self.w, self.sampling)
        return self.decode_packed(torch.from_numpy(buf).to(self.device), offs, cnt, out)

    def decode_packed(self, dev, offs, cnt, out=None):
        """decode() of a batch that pack_streams has packed and that lies on the device already (``dev``)"""
        import torch

        from ._lib import check
        n = cnt["n"]
        if out is None:
            out = torch.empty((n, self.h, self.w, 3), dtype=torch.uint8, device=self.device)
        elif out.dtype != torch.uint8 or tuple(out.shape) != (n, self.h, self.w, 3) or out.device.type != self.device.type:
            raise ValueError(f"out {tuple(out.shape)} {out.dtype} on {out.device}: uint8 [{n}, {self.h}, {self.w}, 3] "
                             f"on {self.device}")
        sn, sy, sx, sc = out.stride()
        if sc != 1 or sx != 3 or sy < 3 * self.w or (n > 1 and sn < sy * (self.h - 1) + 3 * self.w):
            raise ValueError(f"out strides {out.stride()}: channel stride 1, pixel stride 3, rows and frames apart")
        p = dev.data_ptr()
        status = torch.empty((n,), dtype=torch.int32, device=self.device)
        mode = self.mode
        if mode == "auto":                                 # from pack_streams' count: the table is not read back
            mode = "sync" if cnt["max_interval_bytes"] > SYNC_AUTO_BYTES else "wave"
        self.picked = mode
        if mode == "sync":
            need = int(self.lib.s2v_jpeg_decode_sync_ws_bytes(n, self.h, self.w, self.sampling, cnt["data_bytes"],
                                                              cnt["intervals"], self.sub_bytes))
            ws = self._workspace(n, need)
            check(self.lib.s2v_jpeg_decode_sync(
                p + offs["data"], cnt["data_bytes"], p + offs["intervals"], cnt["intervals"], p + offs["frame_first"],
                cnt["max_per_frame"], n, self.h, self.w, self.sampling, p + offs["qtables"], p + offs["huff_sets"],
                cnt["sets"], p + offs["set_index"], out.data_ptr(), sy, sn if n > 1 else 0,
                1 if self.order == "bgr" else 0, status.data_ptr(), ws.data_ptr(), ws.numel(), self.sub_bytes,
                torch.cuda.current_stream(self.device).cuda_stream), "s2v_jpeg_decode_sync")
            return out, status
        ws = self._workspace(n)
        check(self.lib.s2v_jpeg_decode(p + offs["data"], cnt["data_bytes"], p + offs["intervals"], cnt["intervals"],
                                       p + offs["frame_first"], cnt["max_per_frame"], n, self.h, self.w, self.sampling,
                                       p + offs["qtables"], p + offs["huff_sets"], cnt["sets"], p + offs["set_index"],
                                       out.data_ptr(), sy, sn if n > 1 else 0, 1 if self.order == "bgr" else 0,
                                       status.data_ptr(), ws.data_ptr(), ws.numel(), JPEG_DECODE_MODES.index(mode),
                                       torch.cuda.current_stream(self.device).cuda_stream), "s2v_jpeg_decode")
        return out, status


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


class AviReader:
    """RIFF AVI 1.0 with a Motion-JPEG video stream: ``avih``, the ``vids`` stream's ``strh`` / ``strf`` (fps as
    rate / scale, width, height), the frames from ``idx1`` or, without an index, by walking ``movi`` (00dc / 00db
    chunks of the video stream; zero-length ones, dropped frames, are skipped), and the 16-bit PCM of the first
    audio stream if there is one (``pcm`` int16 [frames, channels], ``audio_rate``).  A video stream of another codec
    raises ValueError.  OpenDML files above 2 GiB are not read."""

    def __init__(self, path):
        self.path = str(path)
        with open(self.path, "rb") as f:
            self.data = data = f.read()
        if data[:4] != b"RIFF" or data[8:12] != b"AVI ":
            raise ValueError(f"{self.path}: not a RIFF AVI file")
        self.streams, self.avih = [], None
        self._movi = None                  # (offset of the 'movi' fourcc, end)
        self._idx1 = None
        self._walk(12, min(len(data), 8 + struct.unpack("<I", data[4:8])[0]), None)
        video = [k for k, s in enumerate(self.streams) if s.get("type") == b"vids"]
        if not video or self._movi is None:
            raise ValueError(f"{self.path}: no video stream or no movi list")
        self.video_stream = video[0]
        v = self.streams[self.video_stream]
        fourcc = v.get("compression") or v.get("handler") or b"\0\0\0\0"
        if fourcc not in (b"MJPG", b"mjpg"):
            raise ValueError(f"{self.path}: video codec {fourcc.decode('latin1')!r}; only Motion-JPEG (MJPG) is read: "
                             "transcode with `ffmpeg -i in -c:v mjpeg -q:v 2 -c:a pcm_s16le out.avi`")
        self.w, self.h = v["width"], abs(v["height"])
        self.rate, self.scale = v["rate"], v["scale"]
        if self.rate <= 0 or self.scale <= 0:
            raise ValueError(f"{self.path}: video rate {self.rate} / scale {self.scale}")
        self.fps = self.rate / self.scale
        tags = (b"%02ddc" % self.video_stream, b"%02ddb" % self.video_stream)
        chunks = self._from_index() if self._idx1 is not None else None
        if chunks is None:
            chunks = self._from_movi()
        self._frames = [(o, s) for cc, o, s in chunks if cc in tags and s > 0]
        self.pcm = self.audio_rate = None
        self.channels = 0
        audio = [k for k, s in enumerate(self.streams) if s.get("type") == b"auds"]
        if audio:
            a = self.streams[audio[0]]
            if a.get("format") != 1 or a.get("bits") != 16:
                raise ValueError(f"{self.path}: audio format {a.get('format')} at {a.get('bits')} bits; only 16-bit PCM")
            tag = b"%02dwb" % audio[0]
            raw = b"".join(data[o:o + s] for cc, o, s in chunks if cc == tag)
            self.channels, self.audio_rate = a["channels"], a["audio_rate"]
            self.pcm = np.frombuffer(raw[:len(raw) - len(raw) % (2 * self.channels)], "<i2").reshape(-1, self.channels)

    def _walk(self, i, end, stream):
        data = self.data
        while i + 8 <= end:
            cc, (size,) = data[i:i + 4], struct.unpack("<I", data[i + 4:i + 8])
            body_end = min(end, i + 8 + size)
            if cc == b"LIST":
                kind = data[i + 8:i + 12]
                if kind == b"movi":
                    self._movi = (i + 8, body_end)
                elif kind == b"strl":
                    self.streams.append({})
                    self._walk(i + 12, body_end, self.streams[-1])
                elif kind == b"hdrl":
                    self._walk(i + 12, body_end, None)
            elif cc == b"avih" and size >= 40:
                self.avih = struct.unpack("<10I", data[i + 8:i + 48])
            elif cc == b"strh" and stream is not None and size >= 48:
                stream["type"], stream["handler"] = data[i + 8:i + 12], data[i + 12:i + 16]
                stream["scale"], stream["rate"] = struct.unpack("<II", data[i + 28:i + 36])
            elif cc == b"strf" and stream is not None:
                if stream.get("type") == b"vids" and size >= 40:
                    stream["width"], stream["height"] = struct.unpack("<ii", data[i + 12:i + 20])
                    stream["compression"] = data[i + 24:i + 28]
                elif stream.get("type") == b"auds" and size >= 16:
                    (stream["format"], stream["channels"], stream["audio_rate"], _, _,
                     stream["bits"]) = struct.unpack("<HHIIHH", data[i + 8:i + 24])
            elif cc == b"idx1" and i + 8 + size <= end:       # a cut index is no index: movi is walked
                self._idx1 = (i + 8, body_end)
            i += 8 + size + (size & 1)

    def _from_index(self):
        """[(fourcc, payload offset, size)] from idx1, or None when it does not describe this file: offsets count
        from the 'movi' fourcc or, in some writers' files, from the start of the file."""
        data, (lo, hi), movi = self.data, self._idx1, self._movi[0]
        entries = [struct.unpack("<4sIII", data[k:k + 16]) for k in range(lo, hi - 15, 16)]
        if not entries:
            return None
        for base in (movi, 0):
            o = base + entries[0][2]
            if data[o:o + 4] == entries[0][0] and struct.unpack("<I", data[o + 4:o + 8])[0] == entries[0][3]:
                out = [(cc, base + off + 8, size) for cc, _, off, size in entries]
                if all(o + s <= len(data) for _, o, s in out):
                    return out
        return None

    def _from_movi(self):
        data, out = self.data, []

        def inner(i, end):
            while i + 8 <= end:
                cc, (size,) = data[i:i + 4], struct.unpack("<I", data[i + 4:i + 8])
                if cc == b"LIST":                          # 'rec ' groups
                    inner(i + 12, min(end, i + 8 + size))
                elif i + 8 + size <= end:
                    out.append((cc, i + 8, size))
                i += 8 + size + (size & 1)
        inner(self._movi[0] + 4, self._movi[1])
        return out

    def __len__(self):
        return len(self._frames)

    def frame(self, k: int) -> bytes:
        """the JPEG file of frame k"""
        o, s = self._frames[k]
        return self.data[o:o + s]

    def frames(self, start: int = 0, stop=None) -> list:
        return [self.frame(k) for k in range(start, len(self) if stop is None else min(stop, len(self)))]
