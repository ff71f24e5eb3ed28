"""The "sync" entropy decoder's contract (include/s2v.h, s2v_jpeg_decode_sync) restated in pure Python, and the case
list its tests share.  It does not read csrc/jpeg_dec_core.hpp's code: it works on the unstuffed bytes of an interval
and maps positions to and from the raw (stuffed) byte domain, where the header reads the raw bytes through a
position-tracking bit reader.  Both must give the same states, summaries, statuses and round counts.

  state    (pos, j, k): pos = 8 * (raw byte index in the file) + bit of the next unread bit, canonical (behind the
           last bit of a data 0xFF lies the byte after its stuffed 0x00); j the block within the MCU; k the zigzag
           index, 0: a DC code is next.
  F        ``step``: symbols are decoded while the next starts before the subsequence's end; the fixed rules for
           what the serial decoder calls an error; the block finished on zero bits once the data has run out.
  resolve  ``resolve``: t[0] true, t[b] = (first bit of b, 0, 0), Jacobi rounds t[b + 1] = F_b(t[b]) until a round
           changes nothing; a lane whose entry state did not change is not decoded again.
  write    ``decode_interval``: exclusive scans of the summaries, one more F from the true states.
  status   the error at the lowest block index below count * bpm.
"""
import functools

import numpy as np

import mjpeg_decode_cases as DC

SUB_BYTES = (4, 16, 64, 256, 4096)
OK, BAD_CODE, RUN_PAST_63, DATA_ENDS = 0, 1, 2, 3
ZERO_TAIL = 512                    # bytes of zero bits behind the data: a block finished on them takes < 64 * 32 bits

# the tall streams: at 256 bytes a subsequence the first has more subsequences than a 1024-lane pass takes
TALL_CASES = [("noise", 64, 1048, 0, "none", 100, False), ("mixed", 64, 1048, 2, "none", 75, False)]
CASES = DC.CASES + [c for c in TALL_CASES if c not in DC.CASES]


class Interval:
    """the bytes [s, e) of ``data`` unstuffed, with the maps between raw positions and unstuffed bit indices"""

    def __init__(self, data, s, e):
        raw = data[s:e]
        self.s, self.e = s, e
        u, rawpos, uidx = bytearray(), [], {}
        i = 0
        while i < len(raw):
            uidx[s + i] = len(u)
            rawpos.append(s + i)
            u.append(raw[i])
            if raw[i] == 0xFF:
                assert i + 1 < len(raw) and raw[i + 1] == 0, "a marker inside an interval"
                i += 1
                uidx[s + i] = len(u)                       # a stuffed 0x00 stands for the byte after it
            i += 1
        self.nq = 8 * len(u)
        self.u = bytes(u) + bytes(ZERO_TAIL)
        self.rawpos, self.uidx = rawpos, uidx

    def to_q(self, pos):
        b, bit = pos >> 3, pos & 7
        if b >= self.e:
            return self.nq + pos - 8 * self.e
        return 8 * self.uidx[b] + bit

    def to_pos(self, q):
        if q >= self.nq:
            return 8 * self.e + q - self.nq
        return 8 * self.rawpos[q >> 3] + (q & 7)

    def peek(self, q, n):
        """n <= 16 bits at unstuffed bit index q"""
        i = q >> 3
        u = self.u
        w = (u[i] << 16) | (u[i + 1] << 8) | u[i + 2]
        return (w >> (24 - (q & 7) - n)) & ((1 << n) - 1)


def step(iv, luts, hs, vs, state, sub_begin, sub_end, write=None):
    """F.  -> (exit state, (blocks, [dc sums], err, err_block)).  write: (coef [blocks, 64], first block, total
    blocks, [predictors])"""
    bpm = hs * vs + 2
    pos, j, k = state
    if j >= bpm or k > 63 or pos < 8 * sub_begin:
        pos, j, k = 8 * sub_begin, 0, 0
    stop, last = 8 * sub_end, sub_end >= iv.e
    blocks, dc, err0, err_block = 0, [0, 0, 0], OK, 0
    if pos >= stop and not last:
        return (pos, j, k), (0, dc, OK, 0)
    q = iv.to_q(pos)
    pred = list(write[3]) if write else None
    dry = False
    while True:
        if write and write[1] + blocks >= write[2]:
            break
        if not dry and iv.to_pos(q) >= stop:
            if not last:
                break
            dry = True
        c = 0 if j < hs * vs else j - hs * vs + 1
        (dl, ds), (al, asym) = luts[c]
        blk = write[0][write[1] + blocks] if write else None
        err, close = OK, False
        p16 = iv.peek(q, 16)
        if k == 0:
            n, s = dl[p16], ds[p16]
            if not n:
                err, q = BAD_CODE, q + 1
            elif s > 11:
                err, q, k = BAD_CODE, q + n, 1
            else:
                q += n
                diff = 0
                if s:
                    diff = DC._extend(iv.peek(q, s), s)
                    q += s
                dc[c] += diff
                if write:
                    pred[c] += diff
                    blk[0] = pred[c]
                k = 1
        else:
            n, rs = al[p16], asym[p16]
            if not n:
                err, q = BAD_CODE, q + 1
            else:
                q += n
                r, s = rs >> 4, rs & 15
                if s == 0:
                    if r != 15:
                        close = True
                    elif k + 16 > 63:
                        err, close = RUN_PAST_63, True
                    else:
                        k += 16
                elif k + r > 63:
                    err, close = RUN_PAST_63, True
                else:
                    k += r
                    if write:
                        blk[k] = DC._extend(iv.peek(q, s), s)
                    q += s
                    k += 1
                    close = k == 64
        dry = dry or q > iv.nq
        if dry and not err and close:
            err = DATA_ENDS
        if err and not err0:
            err0, err_block = err, blocks
        if close or (dry and err):
            blocks += 1
            j = 0 if j + 1 == bpm else j + 1
            k = 0
            if dry:
                break
    return (max(iv.to_pos(q), stop), j, k), (blocks, dc, err0, err_block)


def cuts(s, e, sub):
    """[(begin, end)] of the subsequences of [s, e): at least one"""
    n = max(1, -(-(e - s) // sub))
    return [(s + b * sub, min(s + (b + 1) * sub, e)) for b in range(n)]


def resolve(iv, luts, hs, vs, sub):
    """-> (true states t[0 .. nsub], summaries, rounds, first-round exit states)"""
    cs = cuts(iv.s, iv.e, sub)
    n = len(cs)
    t = [(8 * (iv.s + b * sub), 0, 0) for b in range(n + 1)]
    sums = [None] * n
    rounds, first = 0, None
    todo = range(n)                    # the lanes whose entry state changed in the round before: the others keep theirs
    while True:
        new = []
        for b in todo:
            out, sums[b] = step(iv, luts, hs, vs, t[b], cs[b][0], cs[b][1])
            if out != t[b + 1]:
                new.append((b + 1, out))
        for b, out in new:             # Jacobi: a round reads the states of the round before
            t[b] = out
        rounds += 1
        if first is None:
            first = list(t)
        if not new or rounds > n:
            break
        todo = [b for b, _ in new if b < n]
    return t, sums, rounds, first


def decode_interval(iv, luts, hs, vs, sub, count):
    """-> (int64 [count * bpm, 64] coefficients, status, rounds, true states, summaries, first-round states)"""
    bpm = hs * vs + 2
    total = count * bpm
    t, sums, rounds, first = resolve(iv, luts, hs, vs, sub)
    coef = np.zeros((total, 64), np.int64)
    cs = cuts(iv.s, iv.e, sub)
    at, pred, errs = 0, [0, 0, 0], []
    for b, (lo, hi) in enumerate(cs):
        blocks, dc, err, err_block = sums[b]
        if err and at + err_block < total:
            errs.append((at + err_block, err))
        if at < total:
            step(iv, luts, hs, vs, t[b], lo, hi, write=(coef, at, total, pred))
        at += blocks
        pred = [p + d for p, d in zip(pred, dc)]
    return coef, (min(errs)[1] if errs else OK), rounds, t, sums, first


@functools.lru_cache(maxsize=None)
def decode(data, sub):
    """a file -> (coefficients int64 [mcus, bpm, 64], status, [rounds per interval], [per interval (Interval, true
    states, summaries, first-round states)])"""
    p = DC.parse(data)
    hs, vs = p["hs"], p["vs"]
    bpm = hs * vs + 2
    mcus = -(-p["w"] // (8 * hs)) * -(-p["h"] // (8 * vs))
    ri = p["ri"] or mcus
    luts = [(DC._lut(*p["huff"][td]), DC._lut(*p["huff"][0x10 | ta])) for td, ta in p["td_ta"]]
    coef = np.zeros((mcus * bpm, 64), np.int64)
    status, rounds, detail = OK, [], []
    for n, (s, e) in enumerate(DC.intervals(data, p)):
        first, count = n * ri, min(ri, mcus - n * ri)
        iv = Interval(data, s, e)
        c, st, r, t, sums, fr = decode_interval(iv, luts, hs, vs, sub, count)
        coef[first * bpm:(first + count) * bpm] = c
        status = max(status, st)
        rounds.append(r)
        detail.append((iv, t, sums, fr))
    return coef.reshape(mcus, bpm, 64), status, rounds, detail


def checksum(coef):
    """of int16 coefficients in their workspace order: what tools/jpeg_sync_host.cpp prints (FNV-1a, 64 bit, over
    the little-endian bytes)"""
    h = 0xCBF29CE484222325
    for b in np.ascontiguousarray(coef).astype("<i2").tobytes():
        h = ((h ^ b) * 0x100000001B3) & 0xFFFFFFFFFFFFFFFF
    return h
