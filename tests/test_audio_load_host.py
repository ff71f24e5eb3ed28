"""CPU tests of the device audio loader's host side (s2v_amd.audio): the RIFF/WAVE reader against the stdlib ``wave``
and on the files ``wave`` refuses, pcm16 against mjpeg.wav_pcm16, the resampling table against the float64 formula, the
mode names and the parser flag."""
import math
import struct
import wave

import numpy as np
import pytest

import audio_cases as AC
import s2v_import  # noqa: F401
from s2v_amd import _lib, audio, inference, mjpeg

WIDTH = {"u8": 1, "s16": 2, "s24": 3, "s32": 4}
RATE_PAIRS = [(44100, 16000), (48000, 16000), (22050, 16000), (24000, 16000), (8000, 16000), (11025, 16000),
              (16000, 44100)]


def wave_file(path, fmt, rate, channels, n=37, seed=1):
    """An integer file written by the stdlib ``wave`` -> (str(path), codes)"""
    codes = AC.random_codes(fmt, n, channels, seed)
    with wave.open(str(path), "wb") as w:
        w.setnchannels(channels)
        w.setsampwidth(WIDTH[fmt])
        w.setframerate(rate)
        w.writeframes(AC.encode(codes, fmt))
    return str(path), codes


@pytest.mark.parametrize("channels", [1, 2, 3])
@pytest.mark.parametrize("fmt", ["u8", "s16", "s24", "s32"])
def test_read_wav_equals_the_wave_module(tmp_path, fmt, channels):
    path, codes = wave_file(tmp_path / "a.wav", fmt, 22050, channels)
    with wave.open(path, "rb") as w:
        exp = (w.getframerate(), w.getnchannels(), w.getnframes(), w.readframes(w.getnframes()))
    raw, rate, ch, kind, n = audio.read_wav(path)
    assert (rate, ch, n, bytes(raw)) == exp
    assert kind == AC.FORMATS.index(fmt) == getattr(_lib, "PCM_" + fmt.upper())
    assert bytes(raw) == AC.encode(codes, fmt)


@pytest.mark.parametrize("fmt", AC.FORMATS)
@pytest.mark.parametrize("extensible", [False, True])
def test_read_wav_plain_and_extensible_headers(tmp_path, fmt, extensible):
    if fmt in ("f32", "f64"):
        samples = np.random.default_rng(2).uniform(-1, 1, (19, 2))
    else:
        samples = AC.random_codes(fmt, 19, 2, 2)
    path = AC.write(tmp_path / "a.wav", samples, fmt, 24000, extensible=extensible)
    raw, rate, ch, kind, n = audio.read_wav(path)
    assert (rate, ch, kind, n) == (24000, 2, AC.FORMATS.index(fmt), 19)
    assert bytes(raw) == AC.encode(samples, fmt)
    if fmt in ("f32", "f64"):
        with pytest.raises(wave.Error):                       # the gap this reader closes
            wave.open(path, "rb")


def test_read_wav_skips_chunks_and_honours_the_pad_byte(tmp_path):
    codes = AC.random_codes("s16", 11, 1, 3)
    data = AC.encode(codes, "s16")
    before = [AC.chunk(b"LIST", b"INFOISFT" + struct.pack("<I", 5) + b"Lavf\0\0"), AC.chunk(b"fact", b"\x0b\0\0"),
              AC.chunk(b"junk", b"x")]                        # two of odd size: a pad byte each
    p = tmp_path / "a.wav"
    p.write_bytes(AC.wav_bytes(data, "s16", 16000, 1, before=before, after=[AC.chunk(b"LIST", b"INFO")]))
    raw, rate, ch, kind, n = audio.read_wav(str(p))
    assert (rate, ch, n) == (16000, 1, 11) and bytes(raw) == data
    with wave.open(str(p), "rb") as w:
        assert w.readframes(11) == data


@pytest.mark.parametrize("size", [0xFFFFFFFF, 10 ** 6])
def test_read_wav_clamps_a_data_size_past_the_file(tmp_path, size):
    codes = AC.random_codes("s16", 23, 2, 4)
    data = AC.encode(codes, "s16")
    p = tmp_path / "a.wav"
    p.write_bytes(AC.wav_bytes(data, "s16", 44100, 2, data_size=size))
    raw, rate, ch, kind, n = audio.read_wav(str(p))
    assert n == 23 and bytes(raw) == data


def test_read_wav_cuts_to_whole_frames(tmp_path):
    codes = AC.random_codes("s24", 7, 2, 5)
    data = AC.encode(codes, "s24")
    p = tmp_path / "a.wav"
    p.write_bytes(AC.wav_bytes(data + b"\x01\x02\x03\x04\x05", "s24", 48000, 2))
    raw, rate, ch, kind, n = audio.read_wav(str(p))
    assert n == 7 and bytes(raw) == data
    p.write_bytes(AC.wav_bytes(b"", "s24", 48000, 2))         # no frames at all
    raw, rate, ch, kind, n = audio.read_wav(str(p))
    assert n == 0 and len(raw) == 0 and audio.pcm16(str(p))[0].shape == (0, 2)


@pytest.mark.parametrize("name,tag", [("ADPCM", 2), ("A-law", 6), ("µ-law", 7), ("MP3", 0x55), ("unknown", 0x1234)])
def test_read_wav_refuses_compressed_audio_by_name(tmp_path, name, tag):
    p = tmp_path / "a.wav"
    p.write_bytes(AC.wav_bytes(bytes(64), None, 8000, 1, tag=tag, bits=8))
    with pytest.raises(ValueError, match=f"a.wav: unsupported audio format tag 0x{tag:04x} .*{name}"):
        audio.read_wav(str(p))
    p.write_bytes(AC.wav_bytes(bytes(64), None, 8000, 1, tag=tag, bits=8, extensible=True))
    with pytest.raises(ValueError, match=name):
        audio.read_wav(str(p))


def test_read_wav_refusals(tmp_path):
    p = tmp_path / "a.wav"
    good = AC.wav_bytes(bytes(16), "s16", 8000, 2)

    def refused(data, reason):
        p.write_bytes(data)
        with pytest.raises(ValueError, match=f"a.wav: .*{reason}"):
            audio.read_wav(str(p))
    refused(b"RIFX" + good[4:], "not a RIFF/WAVE")
    refused(good[:8] + b"AVI " + good[12:], "not a RIFF/WAVE")
    refused(b"RIFF", "not a RIFF/WAVE")
    refused(good[:12] + good[12 + 24:], "no 'fmt ' chunk")                          # data without fmt
    refused(good[:12], "no 'fmt ' chunk")
    refused(good[:12 + 24], "no 'data' chunk")
    refused(good[:12 + 24] + AC.chunk(b"LIST", b"INFO"), "no 'data' chunk")
    refused(AC.wav_bytes(bytes(16), "s16", 8000, 0), "zero channels")
    refused(AC.wav_bytes(bytes(16), "s16", 0, 2), "zero sample rate")
    refused(AC.wav_bytes(bytes(16), None, 8000, 1, tag=1, bits=12), "sample size of 12 bits")
    refused(AC.wav_bytes(bytes(16), None, 8000, 1, tag=3, bits=16), "sample size of 16 bits")
    refused(b"RIFF" + bytes(4) + b"WAVE" + AC.chunk(b"fmt ", bytes(14)) + AC.chunk(b"data", bytes(4)), "too short")


@pytest.mark.parametrize("fmt", ["u8", "s16", "s24", "s32"])
def test_pcm16_equals_wav_pcm16(tmp_path, fmt):
    path, _ = wave_file(tmp_path / "a.wav", fmt, 11025, 3, n=301)
    got, rate = audio.pcm16(path)
    exp, exp_rate = mjpeg.wav_pcm16(path)
    assert rate == exp_rate == 11025 and got.dtype == exp.dtype == np.int16 and got.shape == exp.shape == (301, 3)
    assert (got == exp).all()


@pytest.mark.parametrize("fmt", ["f32", "f64"])
def test_pcm16_of_float_files(tmp_path, fmt):
    x = np.random.default_rng(6).uniform(-1.2, 1.2, (200, 2)).astype(np.float32 if fmt == "f32" else np.float64)
    x[:6, 0] = [1.0, -1.0, 0.0, 0.5 / 32768, 1.5 / 32768, 32766.5 / 32768]
    got, rate = audio.pcm16(AC.write(tmp_path / "a.wav", x, fmt, 24000))
    assert rate == 24000 and got.dtype == np.int16
    assert (got == np.clip(np.rint(x.astype(np.float64) * 32768), -32768, 32767).astype(np.int16)).all()
    assert got[:6, 0].tolist() == [32767, -32768, 0, 0, 2, 32766]               # rint: halves to even


@pytest.mark.parametrize("sr_in,sr_out", RATE_PAIRS)
def test_resample_table_is_the_formula_rounded_once(sr_in, sr_out):
    table, up, down, half = audio.resample_table(sr_in, sr_out)
    filt, eup, edown, ehalf = AC.filter64(sr_in, sr_out)
    g = math.gcd(sr_in, sr_out)
    assert (up, down) == (eup, edown) == (sr_out // g, sr_in // g)
    assert half == ehalf == int(math.ceil(64 / (0.9475937167399596 * min(1.0, sr_out / sr_in))))
    assert table.dtype == np.float32 and table.shape[0] == up and table.flags.c_contiguous
    assert table.shape[1] % 4 == 0 and 2 * half <= table.shape[1] < 2 * half + 4 and table.ctypes.data % 16 == 0
    assert (table[:, :2 * half] == filt.astype(np.float32)).all() and (table[:, 2 * half:] == 0).all()
    assert audio.resample_table(sr_in, sr_out) is audio.resample_table(sr_in, sr_out)
    assert audio.resample_table(sr_in, sr_out)[0] is table


@pytest.mark.parametrize("sr_in,sr_out", RATE_PAIRS[:3])
def test_table_and_reference_restate_inference_resample(sr_in, sr_out):
    """The float64 reference of the tests is the operation inference.resample defines, and the length is the host's."""
    x = np.random.default_rng(7).uniform(-1, 1, 1500).astype(np.float32)
    exp = inference.resample(x, sr_in, sr_out)
    ref = AC.reference(x, sr_in, sr_out)
    assert len(exp) == len(ref) == AC.host_length(1500, sr_in, sr_out) == audio.resampled_length(1500, sr_in, sr_out)
    assert np.abs(ref - exp).max() <= 2.0 ** -23                 # the host's final rounding to float32
    for n in (0, 1, 2, 159, 160, 441, 44099, 14_000_000):
        assert audio.resampled_length(n, sr_in, sr_out) == AC.host_length(n, sr_in, sr_out)


def test_resample_table_equal_rates_and_the_size_limit():
    assert audio.resample_table(16000, 16000) == (None, 1, 1, 0)
    with pytest.raises(ValueError, match="192001 Hz -> 16000 Hz"):             # 16000 phases x 1624 floats > 2^24
        audio.resample_table(192001, 16000)
    assert audio.resample_table(44099, 16000)[0].size == 16000 * 376 <= audio.TABLE_MAX_FLOATS   # 23 MiB: allowed
    with pytest.raises(ValueError, match="positive"):
        audio.resample_table(0, 16000)


def test_audio_load_mode_names_env_and_flag(monkeypatch):
    monkeypatch.delenv("S2V_AUDIO_LOAD", raising=False)
    assert audio.audio_load_mode() == audio.audio_load_mode("host") == audio.audio_load_mode(None) == "host"
    assert audio.audio_load_mode("device") == "device"
    monkeypatch.setenv("S2V_AUDIO_LOAD", "device")
    assert audio.audio_load_mode(None) == "device" and audio.audio_load_mode("host") == "host"
    monkeypatch.setenv("S2V_AUDIO_LOAD", "")
    assert audio.audio_load_mode(None) == "host"
    monkeypatch.setenv("S2V_AUDIO_LOAD", "gpu")
    with pytest.raises(ValueError, match="S2V_AUDIO_LOAD='gpu'"):
        audio.audio_load_mode(None)
    for bad in ("gpu", "", 1, True):
        with pytest.raises(ValueError, match="audio_load="):
            audio.audio_load_mode(bad)
    ap = inference.build_parser()
    base = ["--face", "f.npy", "--audio", "a.wav"]
    assert ap.parse_args(base).audio_load is None
    assert ap.parse_args(base + ["--audio_load", "device"]).audio_load == "device"
    with pytest.raises(SystemExit):
        ap.parse_args(base + ["--audio_load", "gpu"])


def test_run_refuses_a_bad_mode_before_anything_runs(tmp_path):
    with pytest.raises(ValueError, match="audio_load='gpu'"):
        inference.run(str(tmp_path / "missing.npy"), str(tmp_path / "missing.wav"), audio_load="gpu")


def test_entry_point_refusals_need_no_device():
    lib = _lib.load()
    good = dict(pcm=256, n=100, ch=2, fmt=_lib.PCM_S16, table=256, up=160, down=441, half=187, rs=376, out=256,
                n_out=37)
    assert -(-100 * 160 // 441) == 37

    def call(**kw):
        a = dict(good, **kw)
        return lib.s2v_audio_load(a["pcm"], a["n"], a["ch"], a["fmt"], a["table"], a["up"], a["down"], a["half"],
                                  a["rs"], a["out"], a["n_out"], None)
    for bad, word in ((dict(pcm=None), b"null"), (dict(out=None), b"null"), (dict(table=None), b"null"),
                      (dict(ch=0), b"channels"), (dict(fmt=6), b"format"), (dict(fmt=-1), b"format"),
                      (dict(half=0), b"half"), (dict(rs=373), b"row_stride"), (dict(rs=375), b"aligned"),
                      (dict(table=260), b"aligned"), (dict(n_out=36), b"n_out"), (dict(n_out=38), b"n_out"),
                      (dict(up=0), b"up"), (dict(n=-1), b"negative"), (dict(pcm=257), b"sample size"),
                      (dict(up=1, down=1, n_out=99, table=None), b"n_out"),
                      (dict(up=1, down=4000, half=1 << 20, rs=1 << 21, n_out=1), b"do not fit")):
        assert call(**bad) == -1, bad
        msg = lib.s2v_last_error()
        assert b"audio_load" in msg and word in msg, (bad, msg)
    assert call(n=0, n_out=0, pcm=None, out=None) == 0           # nothing to do: nothing launched
