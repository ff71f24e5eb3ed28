"""Inputs and the NumPy restatement shared by the Motion-JPEG tests (s2v_jpeg_encode, s2v_amd.mjpeg).

``restate`` restates the stream contract of include/s2v.h (s2v_jpeg_encode) in NumPy and plain Python, header
included, without calling s2v_amd.mjpeg: only the Annex K tables (BITS / HUFFVAL and the two base quantisation
tables, which test_mjpeg_host proves equal to Pillow's) are read from there.  It also counts what a stream
exercises, so the byte-equality tests cannot pass on easy inputs.  Results are cached: compute once, share."""
import functools
import math
import struct

import numpy as np

# one MCU; one MCU row, padded on both axes; 10 MCU rows of odd sizes; 66 MCUs in a row (three LDS tiles, two waves)
SHAPES = ((16, 16), (9, 70), (150, 43), (24, 1048))
KINDS = ("zeros", "white", "smooth", "noise", "checker", "mixed")
QUALITIES = (50, 95, 100)
ORDERS = ("bgr", "rgb")


def zigzag_natural():
    """natural index (row * 8 + column) of zigzag position z"""
    out = []
    for s in range(15):
        rows = range(max(0, s - 7), min(7, s) + 1)
        out += [(r, s - r) for r in (rows if s % 2 else reversed(rows))]
    return np.array([r * 8 + c for r, c in out])


ZZ = zigzag_natural()
CI = np.array([[int(np.rint(8192 * (math.sqrt(1 / 8) if u == 0 else 0.5) * math.cos((2 * x + 1) * u * math.pi / 16)))
                for x in range(8)] for u in range(8)], np.int64)


def image(kind, h, w, seed=0):
    """uint8 [h, w, 3]: the three channels differ, so a swapped channel order shows."""
    rng = np.random.default_rng(1000 * h + w + seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    if kind == "zeros":
        return np.zeros((h, w, 3), np.uint8)
    if kind == "white":
        return np.full((h, w, 3), 255, np.uint8)
    if kind == "noise":
        return rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    if kind == "checker":                                   # alternating black and white 8x8 blocks
        return np.repeat((((y // 8 + x // 8) % 2) * 255).astype(np.uint8)[..., None], 3, axis=2)
    smooth = np.stack([127.5 + 127.5 * np.sin(x / 17.0 + y / 29.0 + seed), 255.0 * (x + 2 * y) / max(1, w + 2 * h - 3),
                       127.5 + 127.5 * np.cos(x / 41.0 - y / 13.0)], axis=2)
    if kind == "smooth":
        return np.clip(np.rint(smooth), 0, 255).astype(np.uint8)
    if kind == "mixed":                                     # smooth, with noise right of the middle and a flat band
        out = smooth.copy()
        noise = rng.integers(0, 256, (h, w, 3)).astype(np.float64)
        right = x[..., None] >= w // 2
        out = np.where(right, 0.5 * out + 0.5 * noise, out)
        out[h // 3: h // 3 + max(1, h // 6)] = 200.0
        return np.clip(np.rint(out), 0, 255).astype(np.uint8)
    raise ValueError(kind)


def case_list():
    """(kind, h, w, quality, order): every shape x kind once, qualities and orders cycling, then the streams that
    the coverage list needs at the sizes where they matter."""
    cases, k = [], 0
    for h, w in SHAPES:
        for kind in KINDS:
            cases.append((kind, h, w, QUALITIES[k % 3], ORDERS[(k // 3) % 2]))
            k += 1
    extra = [("noise", 150, 43, 100, "rgb"), ("noise", 24, 1048, 100, "bgr"), ("noise", 9, 70, 50, "rgb"),
             ("smooth", 24, 1048, 100, "rgb"), ("smooth", 150, 43, 100, "bgr"), ("smooth", 150, 43, 50, "rgb"),
             ("checker", 150, 43, 100, "rgb"), ("checker", 24, 1048, 100, "bgr"), ("checker", 16, 16, 100, "bgr"),
             ("mixed", 150, 43, 50, "bgr"), ("mixed", 150, 43, 100, "rgb"), ("mixed", 24, 1048, 95, "rgb"),
             ("mixed", 9, 70, 100, "bgr"), ("white", 24, 1048, 100, "rgb")]
    return cases + [c for c in extra if c not in cases]


CASES = case_list()

# The streams compared with libjpeg's (PSNR against the source, file size): three image kinds at three sizes and
# three qualities.  libjpeg codes a block that lies wholly in the padding as a dummy (the DC of the block before it,
# no AC) where this contract codes the replicated pixels, so a frame made mostly of such blocks (24 rows: a
# third of the luma blocks) is larger by construction; these sizes have few (150x43) or none.
QUALITY_CASES = [(kind, h, w, q, "rgb") for kind in ("smooth", "noise", "mixed")
                 for h, w in ((9, 70), (150, 43), (384, 384)) for q in (50, 90, 100)]


def case_id(c):
    return f"{c[0]}-{c[1]}x{c[2]}-q{c[3]}-{c[4]}"


def quant_tables(quality):
    from s2v_amd import mjpeg
    s = 5000 // quality if quality < 50 else 200 - 2 * quality
    base = np.array([mjpeg.K1_LUMA_ZIGZAG, mjpeg.K2_CHROMA_ZIGZAG], np.int64)
    return np.clip((base * s + 50) // 100, 1, 255)          # [2, 64], zigzag order


def huffman_codes():
    """[DC0, AC0, DC1, AC1] -> {symbol: (code, length)} by T.81 Annex C"""
    from s2v_amd import mjpeg
    tabs = {}
    for tc_th, bits, vals in mjpeg.K3_HUFFMAN:
        code, k, tab = 0, 0, {}
        for length in range(1, 17):
            for _ in range(bits[length - 1]):
                tab[vals[k]] = (code, length)
                code += 1
                k += 1
            code <<= 1
        tabs[tc_th] = tab
    return tabs


def header(h, w, quality):
    from s2v_amd import mjpeg
    qt = quant_tables(quality)

    def seg(marker, body):
        return bytes([0xFF, marker]) + struct.pack(">H", 2 + len(body)) + body
    out = b"\xff\xd8" + seg(0xE0, b"JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00")
    out += seg(0xDB, b"\x00" + bytes(qt[0].tolist())) + seg(0xDB, b"\x01" + bytes(qt[1].tolist()))
    out += seg(0xC0, b"\x08" + struct.pack(">HH", h, w) + b"\x03\x01\x22\x00\x02\x11\x01\x03\x11\x01")
    by_id = {t[0]: t for t in mjpeg.K3_HUFFMAN}
    for tc_th in (0x00, 0x10, 0x01, 0x11):
        out += seg(0xC4, bytes([tc_th]) + by_id[tc_th][1] + by_id[tc_th][2])
    out += seg(0xDD, struct.pack(">H", (w + 15) // 16))
    out += seg(0xDA, b"\x03\x01\x00\x02\x11\x03\x11\x00\x3f\x00")
    return out


def coefficients(img, quality, order):
    """uint8 [h, w, 3] -> quantised int64 coefficients, zigzag order: Y [2 my, 2 mx, 64], Cb and Cr [my, mx, 64]"""
    h, w = img.shape[:2]
    p = np.pad(img, ((0, -h % 16), (0, -w % 16), (0, 0)), mode="edge").astype(np.int64)
    R, G, B = (p[..., 2], p[..., 1], p[..., 0]) if order == "bgr" else (p[..., 0], p[..., 1], p[..., 2])
    Y = np.clip((19595 * R + 38470 * G + 7471 * B + 32768) >> 16, 0, 255)
    Cb = np.clip((-11059 * R - 21709 * G + 32768 * B + 32768 + (128 << 16)) >> 16, 0, 255)
    Cr = np.clip((32768 * R - 27439 * G - 5329 * B + 32768 + (128 << 16)) >> 16, 0, 255)

    def sub(c):
        return (c[0::2, 0::2] + c[0::2, 1::2] + c[1::2, 0::2] + c[1::2, 1::2] + 2) >> 2
    qt = quant_tables(quality)
    out = []
    for plane, t_zz in ((Y, qt[0]), (sub(Cb), qt[1]), (sub(Cr), qt[1])):
        ph, pw = plane.shape
        X = (plane - 128).reshape(ph // 8, 8, pw // 8, 8).transpose(0, 2, 1, 3)          # [by, bx, row, col]
        T = (np.einsum("ur,yxrc->yxuc", CI, X) + 1024) >> 11
        F = (np.einsum("yxuc,vc->yxuv", T, CI) + 16384) >> 15
        t = np.empty(64, np.int64)
        t[ZZ] = t_zz                                                                      # natural order
        t = t.reshape(8, 8)
        q = np.sign(F) * ((np.abs(F) + (t >> 1)) // t)
        q = q.reshape(ph // 8, pw // 8, 64)[..., ZZ]
        q[..., 0] = np.clip(q[..., 0], -1024, 1023)
        q[..., 1:] = np.clip(q[..., 1:], -1023, 1023)
        out.append(q)
    return out


class _Bits:
    def __init__(self):
        self.parts = []

    def put(self, code, length):
        self.parts.append(format(code, "0%db" % length))


def _category(v):
    return int(abs(v)).bit_length()


def _extra(v, cat):
    return (v if v >= 0 else v - 1) & ((1 << cat) - 1)


@functools.lru_cache(maxsize=None)
def _restate_cached(key, quality, order):
    h, w, raw = key
    img = np.frombuffer(raw, np.uint8).reshape(h, w, 3)
    Yq, Cbq, Crq = coefficients(img, quality, order)
    tabs = huffman_codes()
    my, mx = Cbq.shape[:2]
    cnt = {"stuffed": 0, "zrl": 0, "max_ac_cat": 0, "max_dc_cat": 0, "no_eob": 0, "eob_only": 0, "mcu_rows": my,
           "mcus_per_row": mx, "blocks": 0}
    out = [header(h, w, quality)]
    for r in range(my):
        bits = _Bits()
        pred = [0, 0, 0]
        for m in range(mx):
            blocks = [(0, Yq[2 * r, 2 * m]), (0, Yq[2 * r, 2 * m + 1]), (0, Yq[2 * r + 1, 2 * m]),
                      (0, Yq[2 * r + 1, 2 * m + 1]), (1, Cbq[r, m]), (2, Crq[r, m])]
            for comp, blk in blocks:
                dc, ac = tabs[0x00 if comp == 0 else 0x01], tabs[0x10 if comp == 0 else 0x11]
                blk = blk.tolist()
                diff = blk[0] - pred[comp]
                pred[comp] = blk[0]
                cat = _category(diff)
                cnt["max_dc_cat"] = max(cnt["max_dc_cat"], cat)
                bits.put(*dc[cat])
                if cat:
                    bits.put(_extra(diff, cat), cat)
                run = 0
                for k in range(1, 64):
                    v = blk[k]
                    if v == 0:
                        run += 1
                        continue
                    while run > 15:
                        bits.put(*ac[0xF0])
                        cnt["zrl"] += 1
                        run -= 16
                    cat = _category(v)
                    cnt["max_ac_cat"] = max(cnt["max_ac_cat"], cat)
                    bits.put(*ac[(run << 4) | cat])
                    bits.put(_extra(v, cat), cat)
                    run = 0
                if run:
                    bits.put(*ac[0x00])
                cnt["no_eob"] += run == 0
                cnt["eob_only"] += run == 63
                cnt["blocks"] += 1
        s = "".join(bits.parts)
        s += "1" * (-len(s) % 8)
        data = int(s, 2).to_bytes(len(s) // 8, "big")
        cnt["stuffed"] += data.count(b"\xff")
        out.append(data.replace(b"\xff", b"\xff\x00"))
        out.append(bytes([0xFF, 0xD0 + (r & 7)]) if r + 1 < my else b"\xff\xd9")
    return b"".join(out), cnt


def restate(img, quality, order):
    """uint8 [h, w, 3] -> (the JPEG file as bytes, counters)"""
    img = np.ascontiguousarray(img, np.uint8)
    return _restate_cached((img.shape[0], img.shape[1], img.tobytes()), int(quality), order)


def restate_case(c):
    kind, h, w, quality, order = c
    return restate(image(kind, h, w), quality, order)


def pcm_reference(pcm, rate, frames, fps_num, fps_den):
    """the int16 [frames, channels] PCM cut to the duration of ``frames`` video frames at fps_num / fps_den"""
    return pcm[: min(len(pcm), frames * rate * fps_den // fps_num)]


def riff_walk(data):
    """RIFF walker -> (chunks: [(path, fourcc, payload offset, size)], movi fourcc offset).  Checks sizes, padding
    and that every list ends where its parent says."""
    assert data[:4] == b"RIFF" and data[8:12] == b"AVI "
    (riff_size,) = struct.unpack("<I", data[4:8])
    assert riff_size + 8 == len(data) and len(data) % 2 == 0
    chunks, movi = [], [None]

    def inner(start, end, path):
        i = start
        while i < end:
            assert i + 8 <= end
            cc, (size,) = data[i:i + 4], struct.unpack("<I", data[i + 4:i + 8])
            assert i + 8 + size <= end, (path, cc, size)
            if cc == b"LIST":
                kind = data[i + 8:i + 12]
                if kind == b"movi":
                    movi[0] = i + 8
                inner(i + 12, i + 8 + size, path + (kind,))
            else:
                chunks.append((path, cc, i + 8, size))
            i += 8 + size + (size & 1)
            if size & 1:
                assert data[i - 1] == 0
        assert i == end
    inner(12, len(data), ())
    return chunks, movi[0]
