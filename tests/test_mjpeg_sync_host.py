"""The sync entropy decoder's contract (s2v_jpeg_decode_sync) on the host: the pure-Python restatement
(mjpeg_sync_cases) against the serial restatement's coefficients, the coverage of the case list, and the kernels' own
step function (csrc/jpeg_dec_core.hpp, sync_step) compiled into tools/jpeg_sync_host.cpp with AddressSanitizer and
UBSan, which must agree with the restatement on checksum, status and round count.

Bar: EQUALITY with the serial decoder, coefficient for coefficient and status for status, on every case at every
size of mjpeg_sync_cases.SUB_BYTES.  mjpeg_sync_cases.decode is cached, so each (case, size) is decoded once for the
three tests that need it."""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import mjpeg_decode_cases as DC
import mjpeg_sync_cases as SC
import s2v_import  # noqa: F401
from s2v_amd import mjpeg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SERIAL_STATUS = {"bad_code": 1, "run_past_63": 2, "truncated": 3}


@pytest.mark.parametrize("c", SC.CASES, ids=DC.case_id)
def test_restatement_equals_the_serial_decoder(c):
    data = DC.pillow_file(c)
    ref = DC.entropy(data, DC.parse(data))[0]
    for sub in SC.SUB_BYTES:
        coef, status, rounds, detail = SC.decode(data, sub)
        assert status == 0 and np.array_equal(coef, ref), sub
        for r, (iv, t, _, _) in zip(rounds, detail):
            assert r <= len(t)                                           # subsequences + 1


@pytest.mark.parametrize("how", DC.CORRUPTIONS)
def test_restatement_on_damaged_streams(how):
    bad = DC.corrupt(DC.pillow_file(DC.CORRUPT_BASE), how)
    for sub in SC.SUB_BYTES:
        assert SC.decode(bad, sub)[1] == SERIAL_STATUS[how], sub


def padded_tail_file():
    """a stream whose last byte holds no code at 4 bytes a subsequence: every block closes before the last
    subsequence begins, which then holds padding bits alone"""
    for seed in range(64):
        for w in (8, 16, 24):
            data = DC.pillow_encode(DC.image("mixed", 8, w, seed), quality=75, subsampling=0)
            _, status, _, detail = SC.decode(data, 4)
            iv, t, sums, _ = detail[0]
            if len(sums) >= 2 and sum(s[0] for s in sums[:-1]) == (w // 8) * 3:
                return data
    raise AssertionError("no such stream")


def test_the_case_list_reaches_every_hazard():
    """Counted on the true chain of every (case, sub_bytes) the tests decode: at least one of each."""
    hit = dict.fromkeys(("ff_last", "starts_on_stuffed", "pass_through", "block_over_3", "blocks_50", "wrong_j",
                         "wrong_k", "wrong_pos", "short_interval", "rounds_40"), 0)
    for c in SC.CASES:
        data = DC.pillow_file(c)
        for sub in SC.SUB_BYTES:
            _, _, rounds, detail = SC.decode(data, sub)
            hit["rounds_40"] += max(rounds) >= 40
            for iv, t, sums, _ in detail:
                cs = SC.cuts(iv.s, iv.e, sub)
                hit["short_interval"] += iv.e - iv.s < sub
                for b, (lo, hi) in enumerate(cs):
                    hit["ff_last"] += hi < iv.e and data[hi - 1] == 0xFF
                    hit["starts_on_stuffed"] += lo > iv.s and data[lo - 1] == 0xFF and data[lo] == 0
                    blocks = sums[b][0]
                    hit["blocks_50"] += blocks >= 51                     # the first may have begun before the cut
                    if b + 1 < len(cs):
                        hit["pass_through"] += t[b][0] >= 8 * hi
                        hit["block_over_3"] += b > 0 and t[b][2] != 0 and blocks == 0 and t[b][0] < 8 * hi
                    if b > 0:
                        guess = iv.to_pos(iv.to_q(8 * lo))               # canonical
                        pos, j, k = t[b]
                        hit["wrong_j"] += pos == guess and j != 0 and k == 0
                        hit["wrong_k"] += pos == guess and j == 0 and k != 0
                        hit["wrong_pos"] += pos != guess and j == 0 and k == 0
    assert all(hit.values()), hit
    # padding bits that fill the trailing subsequence
    data = padded_tail_file()
    p = DC.parse(data)
    coef, status, _, detail = SC.decode(data, 4)
    assert status == 0 and np.array_equal(coef, DC.entropy(data, p)[0])
    # the batch the device test decodes in one call: three table sets, different lengths and subsequence counts
    counts = {len(SC.decode(f, 64)[3][0][1]) for f in batch_files()}
    assert len(counts) >= 3


def batch_files():
    return [DC.pillow_file(("mixed", 150, 43, 2, r, q, o)) for r, q, o in
            (("none", 75, False), ("none", 5, True), ("none", 100, True), ("none", 75, False))]


# ----------------------------------------------------------------------------- the kernels' step function on the host
def write_job(path, files):
    """the tables file tools/jpeg_decode_host.cpp and tools/jpeg_sync_host.cpp read"""
    info = mjpeg.parse_jpeg(files[0])
    buf, offs, cnt = mjpeg.pack_streams(files, info.h, info.w, info.sampling)
    head = struct.pack("<16i", 0x4A563253, cnt["n"], info.h, info.w, info.sampling, cnt["intervals"],
                       cnt["max_per_frame"], cnt["sets"], offs["intervals"], offs["frame_first"], offs["set_index"],
                       offs["qtables"], offs["huff_sets"], cnt["data_bytes"], 0, 0)
    path.write_bytes(head + buf[:offs["data"]].tobytes())


@pytest.fixture(scope="module")
def host_sync(tmp_path_factory):
    cxx = next((p for p in (shutil.which(n) for n in ("c++", "g++", "clang++")) if p), None)
    if cxx is None:
        pytest.skip("no C++ compiler")
    d = tmp_path_factory.mktemp("jpeg_sync_host")
    exe = d / "jpeg_sync_host"
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    f"{ROOT}/tools/jpeg_sync_host.cpp", "-o", str(exe)], check=True)

    def run(files, sub):
        write_job(d / "tables.bin", files)
        names = []
        for k, f in enumerate(files):
            names.append(str(d / f"{k}.jpg"))
            (d / f"{k}.jpg").write_bytes(f)
        r = subprocess.run([str(exe), str(d / "tables.bin"), str(sub)] + names, capture_output=True, text=True)
        assert r.returncode == 0 and r.stderr == "", r.stderr[-3000:]
        rows = [line.split() for line in r.stdout.splitlines()]
        return (int([v for v in rows if v[0] == "checksum"][0][1], 16), [int(v[2]) for v in rows if v[0] == "status"],
                [int(v[2]) for v in rows if v[0] == "rounds"])
    return run


@pytest.mark.parametrize("c", SC.CASES, ids=DC.case_id)
def test_host_program_equals_the_restatement(host_sync, c):
    data = DC.pillow_file(c)
    for sub in SC.SUB_BYTES:
        coef, status, rounds, _ = SC.decode(data, sub)
        assert host_sync([data], sub) == (SC.checksum(coef), [0], rounds), sub


@pytest.mark.parametrize("how", DC.CORRUPTIONS)
def test_host_program_on_damaged_streams(host_sync, how):
    good = [DC.pillow_file(DC.CORRUPT_BASE), DC.pillow_file(("mixed",) + DC.CORRUPT_BASE[1:])]
    bad = DC.corrupt(good[0], how)
    for sub in SC.SUB_BYTES:
        _, status, rounds = host_sync([good[0], bad, good[1]], sub)
        assert status == [0, SERIAL_STATUS[how], 0], sub
        assert rounds == SC.decode(good[0], sub)[2] + SC.decode(bad, sub)[2] + SC.decode(good[1], sub)[2], sub


def test_host_program_on_a_batch_and_the_padded_tail(host_sync):
    files = batch_files()
    for sub in (4, 64, 256):
        ck, status, rounds = host_sync(files, sub)
        assert status == [0] * 4
        assert ck == SC.checksum(np.concatenate([SC.decode(f, sub)[0] for f in files])), sub
        assert rounds == [r for f in files for r in SC.decode(f, sub)[2]]
    data = padded_tail_file()
    coef, _, rounds, _ = SC.decode(data, 4)
    assert host_sync([data], 4) == (SC.checksum(coef), [0], rounds)
