"""The Motion-JPEG decoder's contract on the host: the restatement (mjpeg_decode_cases.decode) against Pillow, the
coverage of the case list, s2v_amd.mjpeg's parser, marker scan and AVI reader, and the kernels' own arithmetic
(csrc/jpeg_dec_core.hpp) compiled into tools/jpeg_decode_host.cpp with AddressSanitizer and UBSan.

Bar: EQUALITY.  The decoder is integer arithmetic that restates libjpeg-turbo's default decoder (JDCT_ISLOW, fancy
upsampling), which is what Pillow decodes with: every pixel equals PIL.Image.open(...).convert("RGB"), no tolerance.
A damaged stream ends with a non-zero status for its frame, its neighbours untouched, and no sanitizer report."""
import io
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest
from PIL import Image

import mjpeg_cases as MC
import mjpeg_decode_cases as DC
import s2v_import  # noqa: F401
from s2v_amd import mjpeg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def own_file(c):
    kind, h, w, quality, order = c
    return MC.restate(MC.image(kind, h, w), quality, order)[0]


@pytest.mark.parametrize("c", DC.CASES, ids=DC.case_id)
def test_restatement_equals_pillow(c):
    data = DC.pillow_file(c)
    rgb, _ = DC.decode(data)
    ref = DC.pillow_pixels(data)
    assert rgb.shape == ref.shape == (c[1], c[2], 3)
    assert np.array_equal(rgb, ref), f"{int((rgb != ref).any(axis=2).sum())} pixels differ"


@pytest.mark.parametrize("c", DC.OWN_CASES, ids=MC.case_id)
def test_restatement_equals_pillow_on_the_encoder_s_streams(c):
    data = own_file(c)
    assert np.array_equal(DC.decode(data)[0], DC.pillow_pixels(data))


def test_the_case_list_reaches_every_branch():
    """Floors over the Pillow-written cases: at least one of each."""
    cnts = [DC.decode(DC.pillow_file(c))[1] for c in DC.CASES]
    assert sum(c["stuffed"] for c in cnts) >= 1                      # a stuffed 0xFF 0x00
    assert sum(c["zrl"] for c in cnts) >= 1
    assert sum(c["no_eob"] for c in cnts) >= 1                       # a block that ends at coefficient 63
    assert sum(c["eob_only"] for c in cnts) >= 1
    assert max(c["max_ac_cat"] for c in cnts) >= 10
    assert max(c["max_code_len"] for c in cnts) == 16
    assert max(c["intervals"] for c in cnts) > 8                     # the RSTm count wraps
    assert sum(c["straddles"] for c in cnts) >= 1                    # an interval over two MCU rows
    assert sum(c["short_last"] for c in cnts) >= 1
    assert sum(c["optimised"] for c in cnts) >= 1 and sum(not c["optimised"] for c in cnts) >= 1
    assert {c["sampling"] for c in cnts} == {(1, 1), (2, 1), (2, 2)}
    # every size, restart layout and quality of the list, and both replicated-chroma sizes in both subsamplings
    assert {(c[1], c[2]) for c in DC.CASES} == set(DC.SIZES)
    assert {c[4] for c in DC.CASES} == set(DC.RESTARTS) and {c[5] for c in DC.CASES} == set(DC.QUALITIES)
    assert {(c[1], c[2], c[3]) for c in DC.CASES} >= {(7, 4, 1), (7, 4, 2), (3, 3, 1), (3, 3, 2)}


@pytest.mark.parametrize("c", DC.CASES[::3], ids=DC.case_id)
def test_parse_jpeg_and_the_marker_scan(c):
    data = DC.pillow_file(c)
    info, p = mjpeg.parse_jpeg(data), DC.parse(data)
    assert (info.h, info.w) == (c[1], c[2]) and info.sampling == c[3]
    assert info.scan == p["scan"] and info.restart_interval == p["ri"]
    for k in range(3):
        assert np.array_equal(info.qtables[k], p["qt"][p["comps"][k][3]])
        for j, key in enumerate((p["td_ta"][k][0], 0x10 | p["td_ta"][k][1])):
            spec = info.huffman[(2 * k + j) * mjpeg.HUFF_SPEC_BYTES:(2 * k + j + 1) * mjpeg.HUFF_SPEC_BYTES]
            bits, vals = p["huff"][key]
            assert spec[:16] == bits and spec[16:16 + len(vals)] == vals and not any(spec[16 + len(vals):])
    iv = mjpeg.restart_intervals(data, info)
    exp = DC.intervals(data, p)
    ri = info.restart_interval or info.mcus
    assert iv.dtype == np.int32 and [(int(a), int(a + n)) for a, n, _, _ in iv] == exp
    assert iv[:, 2].tolist() == [k * ri for k in range(len(exp))]
    assert int(iv[:, 3].sum()) == info.mcus and int(iv[:, 3].max()) <= ri


def test_a_file_without_dht_gets_the_annex_k_tables():
    data = own_file(DC.OWN_CASES[0])
    i = 2
    out = [data[:2]]
    while data[i + 1] != 0xDA:
        (length,) = struct.unpack(">H", data[i + 2:i + 4])
        if data[i + 1] != 0xC4:
            out.append(data[i:i + 2 + length])
        i += 2 + length
    bare = b"".join(out) + data[i:]
    assert len(bare) < len(data) and mjpeg.parse_jpeg(bare).huffman == mjpeg.parse_jpeg(data).huffman


def test_the_marker_scan_refuses_a_broken_sequence():
    data = DC.pillow_file(("binary", 150, 43, 2, "rows1", 100, False))
    info = mjpeg.parse_jpeg(data)
    iv = mjpeg.restart_intervals(data, info)
    at = int(iv[3, 0]) - 2                                           # the marker before the fourth interval
    assert data[at] == 0xFF and data[at + 1] == 0xD2
    with pytest.raises(ValueError, match="sequence"):
        mjpeg.restart_intervals(data[:at + 1] + b"\xd5" + data[at + 2:], info)
    with pytest.raises(ValueError, match="restart intervals"):
        mjpeg.restart_intervals(data[:at] + data[at + 2:], info)


def _pillow(rgb, **kw):
    buf = io.BytesIO()
    Image.fromarray(rgb).save(buf, "JPEG", **kw)
    return buf.getvalue()


def test_parse_jpeg_refuses_what_the_decoder_does_not_decode():
    rgb = DC.image("mixed", 24, 40)
    with pytest.raises(ValueError, match="progressive"):
        mjpeg.parse_jpeg(_pillow(rgb, progressive=True))
    with pytest.raises(ValueError, match="greyscale"):
        mjpeg.parse_jpeg(_pillow(rgb[..., 0]))
    with pytest.raises(ValueError, match="CMYK"):
        buf = io.BytesIO()
        Image.fromarray(np.concatenate([rgb, rgb[..., :1]], axis=2), "CMYK").save(buf, "JPEG")
        mjpeg.parse_jpeg(buf.getvalue())
    good = _pillow(rgb, quality=75)
    at = good.index(b"\xff\xdb")
    (length,) = struct.unpack(">H", good[at + 2:at + 4])
    assert good[at + 4] >> 4 == 0
    body = good[at + 4:at + 2 + length]
    wide, k = b"", 0
    while k < len(body):                                             # the same tables at 16 bits per entry
        wide += bytes([0x10 | body[k]]) + b"".join(struct.pack(">H", v) for v in body[k + 1:k + 65])
        k += 65
    dqt16 = good[:at] + b"\xff\xdb" + struct.pack(">H", 2 + len(wide)) + wide + good[at + 2 + length:]
    assert Image.open(io.BytesIO(dqt16)).size == (40, 24)            # a file Pillow reads
    with pytest.raises(ValueError, match="16-bit DQT"):
        mjpeg.parse_jpeg(dqt16)
    with pytest.raises(ValueError, match="12-bit"):
        sof = good.index(b"\xff\xc0")
        mjpeg.parse_jpeg(good[:sof + 4] + b"\x0c" + good[sof + 5:])
    with pytest.raises(ValueError, match="sampling"):
        assert good[sof + 11] == 0x22
        mjpeg.parse_jpeg(good[:sof + 11] + b"\x41" + good[sof + 12:])
    with pytest.raises(ValueError, match="SOI"):
        mjpeg.parse_jpeg(b"RIFF")
    assert mjpeg.parse_jpeg(good).sampling == 2


# ----------------------------------------------------------------------------- AVI
@pytest.mark.parametrize("fps, rate, scale", [(25, 25, 1), (30000 / 1001, 30000, 1001), (12.5, 25, 2)])
def test_avi_writer_to_reader(tmp_path, fps, rate, scale):
    files = [DC.pillow_file(("mixed", 150, 43, s, "rows1", 75, False)) for s in (0, 1, 2)] + \
        [DC.pillow_file(("noise", 150, 43, 2, "none", 5, False))]
    t = np.arange(16000) / 8000.0
    pcm = np.stack([np.sin(440 * t), np.cos(300 * t)], axis=1)
    pcm = np.round(pcm * 20000).astype(np.int16)
    path = tmp_path / "a.avi"
    with mjpeg.AviWriter(path, 43, 150, fps, audio=(pcm, 8000)) as avi:
        for f in files:
            avi.write(f)
    r = mjpeg.AviReader(path)
    assert (r.w, r.h, len(r)) == (43, 150, 4) and (r.rate, r.scale) == (rate, scale) and r.fps == rate / scale
    assert r.frames() == files and r.frame(2) == files[2] and r.frames(1, 3) == files[1:3]
    assert r.audio_rate == 8000 and r.channels == 2
    assert np.array_equal(r.pcm, MC.pcm_reference(pcm, 8000, 4, rate, scale))
    # the index cut off (mid-entry and whole): the frames come from walking movi
    data = path.read_bytes()
    at = data.rindex(b"idx1")
    for cut in (at + 20, at):
        short = tmp_path / f"cut{cut - at}.avi"
        short.write_bytes(data[:cut])
        r2 = mjpeg.AviReader(short)
        assert r2.frames() == files and r2.fps == r.fps and np.array_equal(r2.pcm, r.pcm)
    # without audio
    with mjpeg.AviWriter(tmp_path / "v.avi", 43, 150, fps) as avi:
        avi.write(files[0])
    r3 = mjpeg.AviReader(tmp_path / "v.avi")
    assert r3.pcm is None and r3.frames() == files[:1]


def test_avi_reader_names_another_codec(tmp_path):
    path = tmp_path / "a.avi"
    with mjpeg.AviWriter(path, 16, 16, 25) as avi:
        avi.write(own_file(DC.OWN_CASES[0]))
    data = path.read_bytes()
    assert data.count(b"MJPG") == 2
    (tmp_path / "h264.avi").write_bytes(data.replace(b"MJPG", b"H264"))
    with pytest.raises(ValueError, match=r"'H264'.*-c:v mjpeg"):
        mjpeg.AviReader(tmp_path / "h264.avi")
    (tmp_path / "no.avi").write_bytes(b"RIFX" + data[4:])
    with pytest.raises(ValueError, match="not a RIFF AVI"):
        mjpeg.AviReader(tmp_path / "no.avi")


def test_avi_reader_skips_dropped_frames(tmp_path):
    f = own_file(DC.OWN_CASES[0])
    path = tmp_path / "a.avi"
    with mjpeg.AviWriter(path, 16, 16, 25) as avi:
        avi.write(f)
        avi.write(b"")
        avi.write(f)
    assert mjpeg.AviReader(path).frames() == [f, f]


# ----------------------------------------------------------------------------- the kernels' arithmetic on the host
def write_job(path, files):
    """the tables file tools/jpeg_decode_host.cpp reads: a 16-int header, then pack_streams' buffer up to the data"""
    info = mjpeg.parse_jpeg(files[0])
    buf, offs, cnt = mjpeg.pack_streams(files, info.h, info.w, info.sampling)
    head = struct.pack("<16i", 0x4A563253, cnt["n"], info.h, info.w, info.sampling, cnt["intervals"],
                       cnt["max_per_frame"], cnt["sets"], offs["intervals"], offs["frame_first"], offs["set_index"],
                       offs["qtables"], offs["huff_sets"], cnt["data_bytes"], 0, 0)
    path.write_bytes(head + buf[:offs["data"]].tobytes())
    return info


@pytest.fixture(scope="module")
def host_decoder(tmp_path_factory):
    cxx = next((p for p in (shutil.which(n) for n in ("c++", "g++", "clang++")) if p), None)
    if cxx is None:
        pytest.skip("no C++ compiler")
    d = tmp_path_factory.mktemp("jpeg_decode_host")
    exe = d / "jpeg_decode_host"
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    f"{ROOT}/tools/jpeg_decode_host.cpp", "-o", str(exe)], check=True)

    def run(files):
        info = write_job(d / "tables.bin", files)
        names = []
        for k, f in enumerate(files):
            names.append(str(d / f"{k}.jpg"))
            (d / f"{k}.jpg").write_bytes(f)
        r = subprocess.run([str(exe), str(d / "tables.bin"), str(d / "out.rgb")] + names, capture_output=True, text=True)
        assert r.returncode == 0 and r.stderr == "", r.stderr[-3000:]
        status = [int(line.split()[2]) for line in r.stdout.splitlines()]
        return np.fromfile(d / "out.rgb", np.uint8).reshape(len(files), info.h, info.w, 3), status
    return run


@pytest.mark.parametrize("c", DC.CASES, ids=DC.case_id)
def test_host_program_equals_pillow(host_decoder, c):
    data = DC.pillow_file(c)
    px, status = host_decoder([data])
    assert status == [0] and np.array_equal(px[0], DC.pillow_pixels(data))


def test_host_program_on_the_encoder_s_streams_and_mixed_tables(host_decoder):
    for c in DC.OWN_CASES:
        data = own_file(c)
        px, status = host_decoder([data])
        assert status == [0] and np.array_equal(px[0], DC.pillow_pixels(data))
    files = [DC.pillow_file(("mixed", 150, 43, 2, r, q, o)) for r, q, o in
             (("rows1", 75, False), ("none", 5, True), ("blocks3", 100, True))]
    px, status = host_decoder(files)
    assert status == [0, 0, 0]
    for k in range(3):
        assert np.array_equal(px[k], DC.pillow_pixels(files[k]))


@pytest.mark.parametrize("how", DC.CORRUPTIONS)
def test_host_program_on_damaged_streams(host_decoder, how):
    good = [DC.pillow_file(DC.CORRUPT_BASE), DC.pillow_file(("mixed",) + DC.CORRUPT_BASE[1:])]
    px, status = host_decoder([good[0], DC.corrupt(good[0], how), good[1]])
    assert status[0] == 0 and status[2] == 0 and status[1] == {"bad_code": 1, "run_past_63": 2, "truncated": 3}[how]
    assert np.array_equal(px[0], DC.pillow_pixels(good[0])) and np.array_equal(px[2], DC.pillow_pixels(good[1]))
