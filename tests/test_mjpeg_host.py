"""The Motion-JPEG stream contract on the host: the NumPy restatement (mjpeg_cases.restate) against Pillow's
decoder and encoder (libjpeg-turbo), s2v_amd.mjpeg's tables and header against Pillow's segments, and the AVI
writer through a RIFF walker.

Bars.  Decode: every stream opens with the right size and decodes.  Tables: equal to Pillow's DQT / DHT.
Quality: PSNR against the source >= Pillow's own encode (same quality, 4:2:0, optimize=False) - 0.5 dB; the
margin covers libjpeg's chroma downsample rounding and its wider DCT (measured here: at most 0.36 dB below, on
the 9x70 smooth images at quality 90; profiles/mjpeg_quality.json).  Size: <= 1.06 x Pillow's (restart markers and
the padding of each interval's last byte; measured: at most 1.038, 150x43 mixed at quality 50).  Coverage: the byte-equality cases of test_mjpeg_gpu reach every
branch of the entropy coder."""
import io
import struct
import wave

import numpy as np
import pytest
from PIL import Image

import mjpeg_cases as MC
import s2v_import  # noqa: F401
from s2v_amd import mjpeg

ALL = MC.CASES + [c for c in MC.QUALITY_CASES if c not in MC.CASES]


def rgb_of(c):
    img = MC.image(c[0], c[1], c[2])
    return img[..., ::-1] if c[4] == "bgr" else img


def segments(data):
    """[(marker, payload)] of a JPEG file up to SOS"""
    assert data[:2] == b"\xff\xd8"
    i, out = 2, []
    while True:
        assert data[i] == 0xFF
        marker, (length,) = data[i + 1], struct.unpack(">H", data[i + 2:i + 4])
        out.append((marker, data[i + 4:i + 2 + length]))
        i += 2 + length
        if marker == 0xDA:
            return out


def pillow_jpeg(rgb, quality):
    bio = io.BytesIO()
    Image.fromarray(np.ascontiguousarray(rgb)).save(bio, "JPEG", quality=quality, subsampling=2, optimize=False)
    return bio.getvalue()


def phases(c):
    """Images per quality case: enough for 5000 pixels.  A 9x70 image is five MCUs: which way a few coefficients
    round moves its PSNR by several tenths of a dB in either direction (eight phases of the smooth image at
    quality 50: from 0.77 dB below Pillow to 0.68 dB above), so such a case pools eight phases of its image."""
    return -(-5000 // (c[1] * c[2]))


def figures(c):
    """(psnr of the restatement's streams, psnr of Pillow's, size ratio) of one case, pooled over its phases"""
    err, size = [0.0, 0.0], [0, 0]
    for seed in range(phases(c)):
        img = MC.image(c[0], c[1], c[2], seed)
        rgb = img[..., ::-1] if c[4] == "bgr" else img
        for k, d in enumerate((MC.restate(img, c[3], c[4])[0], pillow_jpeg(rgb, c[3]))):
            dec = np.array(Image.open(io.BytesIO(d)).convert("RGB")).astype(np.float64)
            err[k] += float(((dec - rgb) ** 2).sum())
            size[k] += len(d)
    px = phases(c) * c[1] * c[2] * 3
    ps = [float("inf") if e == 0 else 10.0 * np.log10(255.0 ** 2 * px / e) for e in err]
    return ps[0], ps[1], size[0] / size[1]


@pytest.mark.parametrize("c", ALL, ids=MC.case_id)
def test_stream_decodes_in_pillow(c):
    data, cnt = MC.restate_case(c)
    assert data.startswith(mjpeg.jfif_header(c[1], c[2], c[3])) and data.endswith(b"\xff\xd9")
    im = Image.open(io.BytesIO(data))
    assert im.format == "JPEG" and im.size == (c[2], c[1]) and im.mode == "RGB"
    im.load()
    assert np.array(im).shape == (c[1], c[2], 3)
    assert cnt["mcu_rows"] == (c[1] + 15) // 16 and cnt["blocks"] == 6 * cnt["mcu_rows"] * ((c[2] + 15) // 16)
    # the decoded picture is the source, not merely a picture: flat images come back flat
    if c[0] in ("zeros", "white"):
        assert np.abs(np.array(im).astype(int) - rgb_of(c)).max() <= 1


@pytest.mark.parametrize("quality", [50, 75, 95, 100])
def test_tables_and_header_equal_pillow(quality):
    rgb = MC.image("mixed", 40, 56)
    ref = segments(pillow_jpeg(rgb, quality))
    got = segments(mjpeg.jfif_header(40, 56, quality))
    qt = mjpeg.quant_tables(quality)
    assert qt.shape == (2, 64) and np.array_equal(qt, MC.quant_tables(quality))
    assert [p for m, p in got if m == 0xDB] == [p for m, p in ref if m == 0xDB]
    assert [p for m, p in got if m == 0xDB] == [bytes([i]) + bytes(qt[i].tolist()) for i in range(2)]
    assert [p for m, p in got if m == 0xC4] == [p for m, p in ref if m == 0xC4]          # DC0, AC0, DC1, AC1
    assert [p[0] for m, p in got if m == 0xC4] == [0x00, 0x10, 0x01, 0x11]
    assert [p for m, p in got if m in (0xE0, 0xC0)] == [p for m, p in ref if m in (0xE0, 0xC0)]
    assert [m for m, _ in got] == [0xE0, 0xDB, 0xDB, 0xC0, 0xC4, 0xC4, 0xC4, 0xC4, 0xDD, 0xDA]
    assert dict(got)[0xDD] == struct.pack(">H", 4) and dict(got)[0xDA] == bytes([3, 1, 0, 2, 0x11, 3, 0x11, 0, 63, 0])
    assert MC.header(40, 56, quality) == mjpeg.jfif_header(40, 56, quality)


def test_quant_table_rule():
    assert (mjpeg.quant_tables(100) == 1).all()
    assert mjpeg.quant_tables(1).max() == 255 and mjpeg.quant_tables(1).dtype == np.uint16
    assert mjpeg.quant_tables(49)[0, 0] == (16 * (5000 // 49) + 50) // 100
    for bad in (0, 101):
        with pytest.raises(ValueError):
            mjpeg.quant_tables(bad)


@pytest.mark.parametrize("c", MC.QUALITY_CASES, ids=MC.case_id)
def test_quality_and_size_against_pillow(c):
    ours, theirs, ratio = figures(c)
    print(f"{MC.case_id(c)}: psnr {ours:.2f} dB, Pillow {theirs:.2f} dB, size ratio {ratio:.4f}")
    assert ours >= theirs - 0.5
    assert ratio <= 1.06


def test_cases_cover_the_entropy_coder():
    cnts = [MC.restate_case(c)[1] for c in MC.CASES]
    assert max(k["stuffed"] for k in cnts) > 0
    assert max(k["zrl"] for k in cnts) > 0
    assert max(k["max_ac_cat"] for k in cnts) == 10
    assert max(k["max_dc_cat"] for k in cnts) == 11
    assert max(k["no_eob"] for k in cnts) > 0
    assert max(k["eob_only"] for k in cnts) > 0
    assert max(k["mcu_rows"] for k in cnts) > 8                                           # the RST index wraps
    assert max(k["mcus_per_row"] for k in cnts) > 64                                      # more than two LDS tiles
    # the GPU shapes are all there, each with every kind, quality and order somewhere
    assert {(c[1], c[2]) for c in MC.CASES} == set(MC.SHAPES)
    assert {c[0] for c in MC.CASES} == set(MC.KINDS) and {c[3] for c in MC.CASES} == set(MC.QUALITIES)
    assert {c[4] for c in MC.CASES} == set(MC.ORDERS)


def test_channel_order_is_a_swap():
    img = MC.image("mixed", 20, 37)
    assert MC.restate(img, 95, "bgr")[0] == MC.restate(img[..., ::-1], 95, "rgb")[0]
    assert MC.restate(img, 95, "bgr")[0] != MC.restate(img, 95, "rgb")[0]


# ----------------------------------------------------------------------------- AVI
walk = MC.riff_walk


def check_avi(data, streams, fps_num, fps_den, w, h, pcm=None, rate=None):
    chunks, movi = walk(data)
    get = lambda path, cc: [data[o:o + s] for p, c, o, s in chunks if p == path and c == cc]   # noqa: E731
    (avih,) = get((b"hdrl",), b"avih")
    v = struct.unpack("<14I", avih)
    assert v[0] == round(1e6 * fps_den / fps_num) and v[4] == len(streams) and v[6] == (2 if pcm is not None else 1)
    assert v[8:10] == (w, h) and v[3] & 0x10
    strh, strf = get((b"hdrl", b"strl"), b"strh"), get((b"hdrl", b"strl"), b"strf")
    assert len(strh) == len(strf) == v[6]
    sv = struct.unpack("<4s4sIHHIIIIIIII4H", strh[0])
    assert sv[:2] == (b"vids", b"MJPG") and (sv[6], sv[7]) == (fps_den, fps_num) and sv[9] == len(streams)
    bi = struct.unpack("<IiiHH4sIiiII", strf[0])
    assert bi[:6] == (40, w, h, 1, 24, b"MJPG")
    video = [(o, s) for p, c, o, s in chunks if p == (b"movi",) and c == b"00dc"]
    audio = [(o, s) for p, c, o, s in chunks if p == (b"movi",) and c == b"01wb"]
    assert [data[o:o + s] for o, s in video] == list(streams)
    assert sv[10] >= max(len(s) for s in streams)
    for o, s in video:
        im = Image.open(io.BytesIO(data[o:o + s]))
        im.load()
        assert im.size == (w, h)
    if pcm is not None:
        sa = struct.unpack("<4s4sIHHIIIIIIII4H", strh[1])
        ch = pcm.shape[1]
        cut = MC.pcm_reference(pcm, rate, len(streams), fps_num, fps_den)
        assert sa[0] == b"auds" and (sa[6], sa[7]) == (1, rate) and sa[9] == len(cut) and sa[12] == 2 * ch
        wf = struct.unpack("<HHIIHHH", strf[1])
        assert wf == (1, ch, rate, rate * 2 * ch, 2 * ch, 16, 0)
        assert b"".join(data[o:o + s] for o, s in audio) == cut.astype("<i2").tobytes()
        assert 0 < len(audio) <= len(streams)
    else:
        assert not audio
    # idx1: one entry per movi chunk, in order, each pointing at its chunk header
    (idx,) = get((), b"idx1")
    entries = [struct.unpack("<4sIII", idx[i:i + 16]) for i in range(0, len(idx), 16)]
    in_movi = [(c, o, s) for p, c, o, s in chunks if p == (b"movi",)]
    assert len(entries) == len(in_movi) == len(video) + len(audio)
    for (cc, flags, off, size), (c, o, s) in zip(entries, in_movi):
        assert cc == c and cc in (b"00dc", b"01wb") and size == s and movi + off == o - 8
        assert data[movi + off:movi + off + 4] == cc and flags & 0x10
    return chunks


def some_streams(n, h=20, w=36):
    return [MC.restate(MC.image("mixed", h, w, seed=i), 90, "rgb")[0] for i in range(n)]


@pytest.mark.parametrize("fps,num,den", [(25.0, 25, 1), (30000 / 1001, 30000, 1001), (12.5, 25, 2)])
def test_avi_with_audio(tmp_path, fps, num, den):
    rng = np.random.default_rng(5)
    rate = 44100
    pcm = rng.integers(-32768, 32768, (rate // 2, 2)).astype(np.int16)      # 0.5 s: cut at 25 and 29.97 fps, used whole at 12.5
    streams = some_streams(7)
    path = tmp_path / "a.avi"
    wr = mjpeg.AviWriter(path, 36, 20, fps, audio=(pcm, rate))
    for s in streams:
        wr.write(s)
    wr.close()
    wr.close()                                                              # idempotent
    check_avi(path.read_bytes(), streams, num, den, 36, 20, pcm, rate)


def test_avi_audio_shorter_than_video_and_odd_chunks(tmp_path):
    rate = 8000
    pcm = (np.arange(3 * 700).reshape(700, 3) % 30000).astype(np.int16)     # 3 channels, 87.5 ms: under 3 frames
    streams = some_streams(5, 9, 17)
    assert any(len(s) & 1 for s in streams)                                 # an odd chunk is padded
    path = tmp_path / "b.avi"
    with mjpeg.AviWriter(path, 17, 9, 25, audio=(pcm, rate)) as wr:
        for s in streams:
            wr.write(s)
    data = path.read_bytes()
    chunks = check_avi(data, streams, 25, 1, 17, 9, pcm, rate)
    assert sum(1 for p, c, o, s in chunks if c == b"01wb") == 3             # 320 + 320 + 60 sample frames


def test_avi_without_audio(tmp_path):
    streams = some_streams(3)
    path = tmp_path / "c.avi"
    with mjpeg.AviWriter(path, 36, 20, 24) as wr:
        for s in streams:
            wr.write(s)
    check_avi(path.read_bytes(), streams, 24, 1, 36, 20)
    with pytest.raises(ValueError):
        wr.write(streams[0])                                                # closed


def test_avi_refuses_to_pass_the_size_limit(tmp_path):
    streams = some_streams(4)
    assert mjpeg.AVI_MAX_BYTES == 2 ** 31 - 1
    path = tmp_path / "d.avi"
    probe = mjpeg.AviWriter(tmp_path / "probe.avi", 36, 20, 25)
    for s in streams[:2]:
        probe.write(s)
    probe.close()
    two = len((tmp_path / "probe.avi").read_bytes())
    wr = mjpeg.AviWriter(path, 36, 20, 25, max_bytes=two)                   # exactly two frames fit
    wr.write(streams[0])
    wr.write(streams[1])
    with pytest.raises(ValueError, match="2 GiB"):
        wr.write(streams[2])
    wr.close()
    data = path.read_bytes()
    assert len(data) == two
    check_avi(data, streams[:2], 25, 1, 36, 20)                             # the file closed before the limit is whole


def test_wav_pcm16_keeps_rate_and_channels_and_converts_widths(tmp_path):
    rate = 22050
    x = (np.arange(2 * 500).reshape(500, 2) * 37 % 60000 - 30000).astype(np.int16)
    for width in (1, 2, 3, 4):
        if width == 1:
            raw = ((x >> 8) + 128).astype(np.uint8).tobytes()
            exp = ((x >> 8) << 8).astype(np.int16)
        elif width == 2:
            raw, exp = x.astype("<i2").tobytes(), x
        elif width == 3:
            raw = b"".join(struct.pack("<i", int(v) << 8)[:3] for v in x.reshape(-1))
            exp = x
        else:
            raw, exp = (x.astype(np.int32) << 16).astype("<i4").tobytes(), x
        p = tmp_path / f"w{width}.wav"
        with wave.open(str(p), "wb") as f:
            f.setnchannels(2)
            f.setsampwidth(width)
            f.setframerate(rate)
            f.writeframes(raw)
        pcm, got_rate = mjpeg.wav_pcm16(str(p))
        assert got_rate == rate and pcm.dtype == np.int16 and np.array_equal(pcm, exp)
