"""Inputs and the restatement shared by the Motion-JPEG decoder tests (s2v_jpeg_decode, s2v_amd.mjpeg.JpegDecoder).

``decode`` restates the decoder's contract (include/s2v.h, s2v_jpeg_decode) without calling s2v_amd.mjpeg: a
pure-Python baseline parser and Huffman decoder (T.81 F.2.2), then the integer arithmetic in NumPy -- dequantise,
jidctint's ISLOW passes, libjpeg's fancy upsampling over the real chroma size with the cw <= 2 replication rule,
and the colour conversion.  Only the Annex K.3 tables (for a file without DHT) are read from s2v_amd.mjpeg.  It also
counts what a stream exercises, so the equality tests cannot pass on easy inputs.  The reference is Pillow
(libjpeg-turbo: JDCT_ISLOW, fancy upsampling): ``pillow_pixels``.  Results are cached: compute once, share."""
import functools
import io
import struct

import numpy as np

import mjpeg_cases as MC

# one MCU; one MCU row, padded on both axes; odd real chroma size 75x22 over 10 MCU rows; 66 MCUs in a row; the
# sizes where libjpeg replicates chroma instead of filtering it; a single column
SIZES = ((16, 16), (9, 70), (150, 43), (24, 1048), (7, 4), (3, 3), (1, 5))
SAMPLINGS = (0, 1, 2)                                   # Pillow's numbers: 4:4:4, 4:2:2, 4:2:0
RESTARTS = {"none": {}, "blocks1": {"restart_marker_blocks": 1}, "blocks3": {"restart_marker_blocks": 3},
            "rows1": {"restart_marker_rows": 1}}
QUALITIES = (5, 75, 100)
KINDS = ("mixed", "noise", "smooth", "binary")


def image(kind, h, w, seed=0):
    """uint8 RGB [h, w, 3]; "binary" is black / white noise, whose blocks carry the largest AC coefficients"""
    if kind == "binary":
        rng = np.random.default_rng(7000 * h + w + seed)
        return (rng.integers(0, 2, (h, w, 3), dtype=np.uint8) * 255).astype(np.uint8)
    return MC.image(kind, h, w, seed)


def case_list():
    """(kind, h, w, sampling, restart, quality, optimize): every size x sampling twice, with the restart layouts,
    qualities, image kinds and ``optimize`` cycling at coprime periods, then the streams the coverage floors and
    the issue's list need at the sizes where they matter."""
    cases, k = [], 0
    names = list(RESTARTS)
    for rep in range(2):
        for h, w in SIZES:
            for s in SAMPLINGS:
                cases.append((KINDS[k % 4], h, w, s, names[(k + rep) % 4], QUALITIES[k % 3], k % 5 == 0))
                k += 1
    extra = [("binary", 150, 43, 2, "rows1", 100, False), ("binary", 24, 1048, 2, "blocks3", 100, False),
             ("binary", 24, 1048, 0, "none", 75, True), ("noise", 150, 43, 1, "blocks3", 100, False),
             ("noise", 150, 43, 2, "blocks1", 75, True), ("zeros", 150, 43, 2, "rows1", 75, False),
             ("white", 9, 70, 1, "blocks3", 5, False), ("noise", 16, 16, 2, "none", 5, True),
             ("smooth", 150, 43, 0, "rows1", 5, False), ("mixed", 24, 1048, 1, "rows1", 75, True),
             ("binary", 7, 4, 2, "blocks1", 100, False), ("binary", 3, 3, 1, "none", 100, False),
             ("binary", 3, 3, 2, "none", 75, True), ("noise", 1, 5, 2, "blocks1", 100, False)]
    return cases + [c for c in extra if c not in cases]


CASES = case_list()
# the project's own encoder's streams (MC.restate: its contract on the CPU) the device tests decode, at three of
# MC.SHAPES: (kind, h, w, quality, order)
OWN_CASES = [("smooth", 16, 16, 50, "rgb"), ("mixed", 150, 43, 95, "bgr"), ("noise", 24, 1048, 100, "rgb")]


def case_id(c):
    return f"{c[0]}-{c[1]}x{c[2]}-s{c[3]}-{c[4]}-q{c[5]}" + ("-opt" if c[6] else "")


@functools.lru_cache(maxsize=None)
def pillow_file(c):
    """the JPEG file Pillow writes for a case"""
    from PIL import Image
    kind, h, w, sampling, restart, quality, optimize = c
    buf = io.BytesIO()
    Image.fromarray(image(kind, h, w)).save(buf, "JPEG", quality=quality, subsampling=sampling, optimize=optimize,
                                            **RESTARTS[restart])
    return buf.getvalue()


def pillow_encode(rgb, **kw):
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(np.ascontiguousarray(rgb)).save(buf, "JPEG", **kw)
    return buf.getvalue()


@functools.lru_cache(maxsize=None)
def _pillow_pixels(data):
    from PIL import Image
    a = np.asarray(Image.open(io.BytesIO(data)).convert("RGB")).copy()
    a.setflags(write=False)
    return a


def pillow_pixels(data):
    """the reference: uint8 RGB [h, w, 3] (read-only, shared)"""
    return _pillow_pixels(bytes(data))


# ----------------------------------------------------------------------------- the restatement
def parse(data):
    """dict(h, w, hs, vs, qt {id: int64[64] zigzag}, comps [(id, h, v, tq)], huff {tc_th: (bits, vals)}, ri,
    scan (start, end), td_ta [(td, ta)]) of a baseline file"""
    assert data[:2] == b"\xff\xd8"
    out = {"qt": {}, "huff": {}, "ri": 0}
    i = 2
    while True:
        assert data[i] == 0xFF, i
        m = data[i + 1]
        (length,) = struct.unpack(">H", data[i + 2:i + 4])
        body = data[i + 4:i + 2 + length]
        i += 2 + length
        if m == 0xDB:
            k = 0
            while k < len(body):
                assert body[k] >> 4 == 0
                out["qt"][body[k] & 15] = np.array(list(body[k + 1:k + 65]), np.int64)
                k += 65
        elif m == 0xC0:
            prec, out["h"], out["w"], nc = struct.unpack(">BHHB", body[:6])
            assert prec == 8 and nc == 3
            out["comps"] = [(body[6 + 3 * c], body[7 + 3 * c] >> 4, body[7 + 3 * c] & 15, body[8 + 3 * c])
                            for c in range(3)]
        elif m == 0xC4:
            k = 0
            while k < len(body):
                bits = body[k + 1:k + 17]
                out["huff"][body[k]] = (bytes(bits), bytes(body[k + 17:k + 17 + sum(bits)]))
                k += 17 + sum(bits)
        elif m == 0xDD:
            (out["ri"],) = struct.unpack(">H", body[:2])
        elif m == 0xDA:
            assert body[0] == 3 and tuple(body[7:]) == (0, 63, 0)
            out["td_ta"] = [(body[2 + 2 * c] >> 4, body[2 + 2 * c] & 15) for c in range(3)]
            break
        else:
            assert m not in (0xC1, 0xC2, 0xC3, 0xC9, 0xCA), hex(m)
    if not out["huff"]:
        from s2v_amd import mjpeg
        out["huff"] = {t: (b, v) for t, b, v in mjpeg.K3_HUFFMAN}
    end = i
    while not (data[end] == 0xFF and data[end + 1] != 0 and not 0xD0 <= data[end + 1] <= 0xD7):
        end += 1
    out["scan"] = (i, end)
    out["hs"], out["vs"] = out["comps"][0][1:3]
    assert all(c[1:3] == (1, 1) for c in out["comps"][1:])
    return out


def intervals(data, p):
    """[(start, end)] of the restart intervals, markers excluded, with the RSTm sequence checked"""
    s, e = p["scan"]
    out, begin, m, i = [], s, 0, s
    while i < e - 1:
        if data[i] == 0xFF and 0xD0 <= data[i + 1] <= 0xD7:
            assert data[i + 1] == 0xD0 + m % 8
            out.append((begin, i))
            begin, m, i = i + 2, m + 1, i + 2
        else:
            i += 1
    return out + [(begin, e)]


@functools.lru_cache(maxsize=None)
def _lut(bits, vals):
    """16-bit look-up of a Huffman table: (length list, symbol list), length 0 where no code leads the 16 bits"""
    length, sym = np.zeros(65536, np.int64), np.zeros(65536, np.int64)
    code, k = 0, 0
    for n in range(1, 17):
        for _ in range(bits[n - 1]):
            lo = code << (16 - n)
            length[lo:lo + (1 << (16 - n))] = n
            sym[lo:lo + (1 << (16 - n))] = vals[k]
            code, k = code + 1, k + 1
        code <<= 1
    return length.tolist(), sym.tolist()


def _extend(v, s):
    return v - (1 << s) + 1 if v < (1 << (s - 1)) else v


def entropy(data, p):
    """-> (int64 coefficients [mcus, blocks per MCU, 64] in zigzag order, counters)"""
    hs, vs = p["hs"], p["vs"]
    bpm = hs * vs + 2
    mcols, mrows = -(-p["w"] // (8 * hs)), -(-p["h"] // (8 * vs))
    mcus = mcols * mrows
    ri = p["ri"] or mcus
    ivs = intervals(data, p)
    assert len(ivs) == -(-mcus // ri)
    coef = np.zeros((mcus, bpm, 64), np.int64)
    from s2v_amd import mjpeg
    annex_k = {t: (b, v) for t, b, v in mjpeg.K3_HUFFMAN}
    cnt = {"stuffed": 0, "zrl": 0, "no_eob": 0, "eob_only": 0, "max_ac_cat": 0, "max_code_len": 0,
           "intervals": len(ivs), "straddles": 0, "short_last": int(mcus % ri != 0),
           "optimised": int(any(p["huff"][t] != annex_k.get(t) for t in p["huff"])), "sampling": (hs, vs)}
    luts = []
    for c in range(3):
        td, ta = p["td_ta"][c]
        luts.append((_lut(*p["huff"][td]), _lut(*p["huff"][0x10 | ta])))
    for n, (s, e) in enumerate(ivs):
        first, count = n * ri, min(ri, mcus - n * ri)
        cnt["straddles"] += first // mcols != (first + count - 1) // mcols
        raw = data[s:e]
        cnt["stuffed"] += raw.count(b"\xff\x00")
        raw = raw.replace(b"\xff\x00", b"\xff")
        nbits = 8 * len(raw)
        v = int.from_bytes(raw, "big") << 32                  # zero bits past the end for the 16-bit peek
        total = nbits + 32
        pos = 0
        pred = [0, 0, 0]
        for m in range(first, first + count):
            for j in range(bpm):
                c = 0 if j < hs * vs else j - hs * vs + 1
                (dl, ds), (al, asym) = luts[c]
                blk = coef[m, j]
                peek = (v >> (total - pos - 16)) & 0xFFFF
                n_, s_ = dl[peek], ds[peek]
                assert n_
                pos += n_
                if s_:
                    pred[c] += _extend((v >> (total - pos - s_)) & ((1 << s_) - 1), s_)
                    pos += s_
                blk[0] = pred[c]
                k, eob = 1, False
                while k < 64:
                    peek = (v >> (total - pos - 16)) & 0xFFFF
                    n_, rs = al[peek], asym[peek]
                    assert n_
                    pos += n_
                    cnt["max_code_len"] = max(cnt["max_code_len"], n_)
                    r, s_ = rs >> 4, rs & 15
                    if s_ == 0:
                        if r != 15:
                            eob = True
                            cnt["eob_only"] += k == 1
                            break
                        cnt["zrl"] += 1
                        k += 16
                        continue
                    k += r
                    assert k < 64
                    blk[k] = _extend((v >> (total - pos - s_)) & ((1 << s_) - 1), s_)
                    pos += s_
                    cnt["max_ac_cat"] = max(cnt["max_ac_cat"], s_)
                    k += 1
                cnt["no_eob"] += not eob
                assert pos <= nbits
    return coef, cnt


def _islow_pass(i):
    """jidctint's 1-D pass on a list of eight int64 arrays, without the rounding shift"""
    z1 = (i[2] + i[6]) * 4433
    t2, t3 = z1 - i[6] * 15137, z1 + i[2] * 6270
    t0, t1 = (i[0] + i[4]) << 13, (i[0] - i[4]) << 13
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    a, b, c, d = i[7], i[5], i[3], i[1]
    z1, z2, z3, z4 = a + d, b + c, a + c, b + d
    z5 = (z3 + z4) * 9633
    a, b, c, d = a * 2446, b * 16819, c * 25172, d * 12299
    z1, z2, z3, z4 = z1 * -7373, z2 * -20995, z3 * -16069 + z5, z4 * -3196 + z5
    a, b, c, d = a + z1 + z3, b + z2 + z4, c + z2 + z3, d + z1 + z4
    return [t10 + d, t11 + c, t12 + b, t13 + a, t13 - a, t12 - b, t11 - c, t10 - d]


def idct(coef_zz, q_zz):
    """int64 [..., 64] zigzag coefficients, int64 [64] zigzag table -> uint8-range int64 [..., 8, 8] samples"""
    nat = np.zeros(coef_zz.shape, np.int64)
    nat[..., MC.ZZ] = coef_zz * q_zz
    x = nat.reshape(coef_zz.shape[:-1] + (8, 8))
    cols = _islow_pass([x[..., r, :] for r in range(8)])                     # down the columns
    t = np.stack([(c + 1024) >> 11 for c in cols], axis=-2)
    rows = _islow_pass([t[..., :, c] for c in range(8)])                     # along the rows
    y = np.stack([(r + (1 << 17)) >> 18 for r in rows], axis=-1)
    return np.clip(y + 128, 0, 255)


def upsample(c, hs, vs, h, w):
    """real-size chroma int64 [ch, cw] -> [h, w]: libjpeg's fancy filters, replication when cw <= 2"""
    ch, cw = c.shape
    if hs == 1:
        return c[:h, :w]
    if cw <= 2:
        return np.repeat(np.repeat(c, vs, axis=0), 2, axis=1)[:h, :w]
    if vs == 2:
        up = c[[0] + list(range(ch - 1))]
        down = c[list(range(1, ch)) + [ch - 1]]
        s = np.empty((2 * ch, cw), np.int64)
        s[0::2], s[1::2] = 3 * c + up, 3 * c + down
        three, r0, r1, sh = 3 * s, 8, 7, 4
    else:
        s, three, r0, r1, sh = c, 3 * c, 1, 2, 2
    left = s[:, [0] + list(range(cw - 1))]
    right = s[:, list(range(1, cw)) + [cw - 1]]
    out = np.empty((s.shape[0], 2 * cw), np.int64)
    out[:, 0::2] = (three + left + r0) >> sh
    out[:, 1::2] = (three + right + r1) >> sh
    return out[:h, :w]


@functools.lru_cache(maxsize=None)
def _decode(data):
    p = parse(data)
    coef, cnt = entropy(data, p)
    h, w, hs, vs = p["h"], p["w"], p["hs"], p["vs"]
    mcols, mrows = -(-w // (8 * hs)), -(-h // (8 * vs))
    planes = []
    for c in range(3):
        q = p["qt"][p["comps"][c][3]]
        if c == 0:
            px = idct(coef[:, :hs * vs], q).reshape(mrows, mcols, vs, hs, 8, 8)
            planes.append(px.transpose(0, 2, 4, 1, 3, 5).reshape(mrows * vs * 8, mcols * hs * 8))
        else:
            px = idct(coef[:, hs * vs + c - 1], q).reshape(mrows, mcols, 8, 8)
            planes.append(px.transpose(0, 2, 1, 3).reshape(mrows * 8, mcols * 8))
    ch, cw = -(-h // vs), -(-w // hs)
    Y = planes[0][:h, :w]
    cb = upsample(planes[1][:ch, :cw], hs, vs, h, w) - 128
    cr = upsample(planes[2][:ch, :cw], hs, vs, h, w) - 128
    R = np.clip(Y + ((91881 * cr + 32768) >> 16), 0, 255)
    G = np.clip(Y + ((-22554 * cb - 46802 * cr + 32768) >> 16), 0, 255)
    B = np.clip(Y + ((116130 * cb + 32768) >> 16), 0, 255)
    rgb = np.stack([R, G, B], axis=2).astype(np.uint8)
    rgb.setflags(write=False)
    return rgb, cnt


def decode(data):
    """a baseline JPEG file -> (uint8 RGB [h, w, 3] read-only, counters)"""
    return _decode(bytes(data))


# ----------------------------------------------------------------------------- damaged streams
CORRUPTIONS = ("truncated", "bad_code", "run_past_63")
CORRUPT_BASE = ("noise", 40, 56, 2, "rows1", 75, False)      # Annex K tables, three intervals of four MCUs


def corrupt(data, how):
    """``data`` (a file with restart markers and the Annex K tables) with its middle interval damaged, the markers
    and every other interval as they were:
      truncated    the interval's second half is cut away: its data ends early;
      bad_code     sixteen bytes become 0xFF 0x00 x 8, sixty-four 1-bits: whatever symbol they begin in takes 31 of
                   them at the most, and sixteen 1-bits lead no code of any table;
      run_past_63  the interval is replaced by a DC code of category 0 and four ZRL codes."""
    p = parse(data)
    ivs = intervals(data, p)
    assert len(ivs) >= 3
    s, e = ivs[len(ivs) // 2]
    if how == "truncated":
        cut = s + (e - s) // 2
        if data[cut - 1] == 0xFF:
            cut -= 1
        return data[:cut] + data[e:]
    if how == "bad_code":
        for at in range(s + (e - s) // 4, e - 18):
            if 0xFF not in data[at - 1:at + 17]:
                return data[:at] + b"\xff\x00" * 8 + data[at + 16:]
        raise AssertionError("no window without 0xFF")
    if how == "run_past_63":
        bits = "00" + "11111111001" * 4                      # Annex K luma: DC category 0, AC 0xF0
        bits += "1" * (-len(bits) % 8)
        body = int(bits, 2).to_bytes(len(bits) // 8, "big").replace(b"\xff", b"\xff\x00")
        return data[:s] + body + data[e:]
    raise ValueError(how)
