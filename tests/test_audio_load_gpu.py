"""s2v_audio_load (csrc/audio.hip) through s2v_amd.audio.load_audio, and the CLI's --audio_load device.

Bars.  BIT-EQUAL wherever fp32 gives one answer: the decode + downmix pass against inference.load_wav / NumPy, and
clips of isolated +-1.0 impulses against the array built on the host from the fp32 table (one exact product per
output, exact zeros elsewhere), over impulses that reach every (phase, tap) pair of the table and over a clip whose
indices pass 2^31.  Against the float64 reference (audio_cases.reference) the bound is the derived fp32 one,
audio_cases.tolerance: gamma_m * max_p sum_t |table[p][t]| * max|x| with m = 2 half + 2 (5.3e-5 for full-scale input
at 44.1 kHz; a sequential fp32 evaluation on a CPU stays at 9e-7).  Every call writes into a view of a sentinel-filled
buffer whose margins must keep the sentinel."""
import json
import os
import wave

import numpy as np
import pytest
import torch

import audio_cases as AC
import mjpeg_cases as MC
import s2v_import  # noqa: F401
from conftest import GOLDEN

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENTINEL = -123456.0
PAD = 1024                                                                 # floats on either side of the view
AUDIO_1 = os.path.join(GOLDEN, "examples", "audio_1.wav")
IMPULSE_PAIRS = [(44100, 16000), (48000, 16000), (22050, 16000), (8000, 16000), (11025, 16000), (16000, 44100)]


def load(path, sr=16000):
    """load_audio(path, sr) into a view of a sentinel-filled buffer -> float32 [n_out] (NumPy), after checking the
    margins"""
    from s2v_amd import audio
    _, rate, _, _, n = audio.read_wav(path)
    n_out = audio.resampled_length(n, rate, sr)
    buf = torch.full((n_out + 2 * PAD,), SENTINEL, dtype=torch.float32, device=DEV)
    out = audio.load_audio(path, sr, out=buf[PAD:PAD + n_out])
    assert out.data_ptr() == buf.data_ptr() + 4 * PAD and out.shape == (n_out,)
    host = buf.cpu().numpy()
    assert (host[:PAD] == SENTINEL).all() and (host[PAD + n_out:] == SENTINEL).all()
    return host[PAD:PAD + n_out].copy()


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ----------------------------------------------------------------------------- decode + downmix
@pytest.mark.parametrize("channels", [1, 2, 3, 6])
@pytest.mark.parametrize("fmt", ["u8", "s16", "s24", "s32"])
def test_passthrough_equals_load_wav(tmp_path, fmt, channels):
    from s2v_amd import inference
    codes = AC.random_codes(fmt, 4099, channels, seed=channels)            # 17 workgroups, the last one ragged
    path = AC.write(tmp_path / "a.wav", codes, fmt, 16000)
    exp = inference.load_wav(path, 16000)
    got = load(path)
    assert got.shape == exp.shape == (4099,) and exp.dtype == np.float32
    assert (bits(got) == bits(exp)).all()
    assert (bits(exp) == bits(AC.decode(codes, fmt).mean(axis=1))).all()   # the statement the float formats use


@pytest.mark.parametrize("channels", [1, 2, 3, 6])
@pytest.mark.parametrize("fmt", ["f32", "f64"])
@pytest.mark.parametrize("extensible", [False, True])
def test_passthrough_of_float_files(tmp_path, fmt, channels, extensible):
    x = np.random.default_rng(channels).uniform(-1, 1, (4099, channels))
    x.reshape(-1)[:4] = [1.0, -1.0, 0.0, 1.0 - 2.0 ** -30]                # the last rounds to 1.0 as float32
    x = x.astype(np.float32) if fmt == "f32" else x
    got = load(AC.write(tmp_path / "a.wav", x, fmt, 16000, extensible=extensible))
    assert (bits(got) == bits(AC.decode(x, fmt).mean(axis=1))).all()


# ----------------------------------------------------------------------------- indexing: impulses
@pytest.mark.parametrize("sr_in,sr_out", IMPULSE_PAIRS)
def test_impulses_reach_every_tap_and_equal_the_table(tmp_path, sr_in, sr_out):
    from s2v_amd import audio
    table, up, down, half = audio.resample_table(sr_in, sr_out)
    s = AC.impulse_spacing(down, half)
    positions = np.arange(1501, dtype=np.int64) * s                        # the first sample ... the last sample
    values = np.where(np.arange(1501) % 2 == 0, 1.0, -1.0)
    n = int(positions[-1]) + 1
    x = np.zeros((n, 1), np.float32)
    x[positions, 0] = values
    n_out = AC.host_length(n, sr_in, sr_out)
    exp, reached = AC.impulse_response(table, up, down, half, positions.tolist(), values.tolist(), n_out)
    assert reached.shape == (up, 2 * half) and reached.all()               # the complete table
    got = load(AC.write(tmp_path / "a.wav", x, "f32", sr_in), sr_out)
    assert got.shape == (n_out,)
    bad = np.nonzero(got != exp)[0]
    assert len(bad) == 0, (len(bad), bad[:8], got[bad[:8]], exp[bad[:8]])
    assert np.count_nonzero(got) == np.count_nonzero(exp) > 0.9 * 1501 * 2 * half * up / down


def test_long_clip_indices_pass_2_to_31(tmp_path):
    from s2v_amd import audio
    table, up, down, half = audio.resample_table(44100, 16000)
    n = 14_000_000
    cross = (1 << 31) // up                                                # the input under the output with k down = 2^31
    positions = [cross - 1000, cross, cross + 1000, n - 1]
    codes = np.full((n, 1), 128, np.uint8)
    codes[positions, 0] = 0                                                # -1.0 exactly
    n_out = AC.host_length(n, 44100, 16000)
    exp, _ = AC.impulse_response(table, up, down, half, positions, [-1.0] * 4, n_out)
    k = np.nonzero(AC.impulse_response(table, up, down, half, [cross], [-1.0], n_out)[0])[0]
    assert k.min() * down < 1 << 31 < k.max() * down and n_out == 5_079_366  # one impulse's outputs straddle 2^31
    got = load(AC.write(tmp_path / "a.wav", codes, "u8", 44100))
    bad = np.nonzero(got != exp)[0]
    assert len(bad) == 0, (len(bad), bad[:8], got[bad[:8]], exp[bad[:8]])


# ----------------------------------------------------------------------------- edges, tiles, accuracy
@pytest.mark.parametrize("sr_in", [44100, 8000])
def test_short_clips_and_tile_edges(tmp_path, sr_in):
    from s2v_amd import audio, inference
    table, up, down, half = audio.resample_table(sr_in, 16000)
    tile_in = 1024 * down // up                                            # the inputs under one tile of 1024 outputs
    rng = np.random.default_rng(sr_in)
    lengths = [1, 2, half - 1, 2 * half, tile_in - 1, tile_in, tile_in + 1]
    assert {AC.host_length(n, sr_in, 16000) for n in lengths[-3:]} >= {1024, 1024 + (2 if up == 2 else 1)}
    for n in lengths:
        x = rng.uniform(-1, 1, (n, 1)).astype(np.float32)
        got = load(AC.write(tmp_path / f"a{n}.wav", x, "f32", sr_in))
        assert len(got) == AC.host_length(n, sr_in, 16000) == len(inference.resample(x[:, 0], sr_in, 16000))
        err = np.abs(got - AC.reference(x[:, 0], sr_in, 16000)).max()
        assert err <= AC.tolerance(table, half, np.abs(x).max()), (n, err)


@pytest.mark.parametrize("sr_in", [44100, 8000])
def test_outputs_do_not_depend_on_samples_beyond_their_taps(tmp_path, sr_in):
    from s2v_amd import audio
    table, up, down, half = audio.resample_table(sr_in, 16000)
    rng = np.random.default_rng(11)
    x = rng.uniform(-1, 1, (9000 * down // up, 1)).astype(np.float32)      # nine tiles, the last one ragged
    n = len(x) - 2 * half - 301
    short = load(AC.write(tmp_path / "a.wav", x[:n], "f32", sr_in))
    full = load(AC.write(tmp_path / "b.wav", x, "f32", sr_in))
    k = np.arange(len(short), dtype=np.int64)
    inside = k * down // up + half <= n - 1                               # the last tap lies in the shorter clip
    assert 0 < inside.sum() < len(short) < len(full)
    assert (bits(short[inside]) == bits(full[:len(short)][inside])).all()
    assert (short[~inside] != full[:len(short)][~inside]).any()


@pytest.mark.parametrize("case", ["s16 stereo 44.1 kHz", "f32 mono 22.05 kHz"])
def test_accuracy_against_float64(tmp_path, case):
    from s2v_amd import audio
    rng = np.random.default_rng(5)
    if case.startswith("s16"):
        sr_in, fmt = 44100, "s16"
        samples = AC.random_codes("s16", 2 * sr_in, 2, seed=5)
    else:
        sr_in, fmt = 22050, "f32"
        samples = rng.uniform(-1, 1, (2 * sr_in, 1)).astype(np.float32)
    table, up, down, half = audio.resample_table(sr_in, 16000)
    x = AC.decode(samples, fmt).astype(np.float64).mean(axis=1)            # exact: the fp32 downmix of s16 pairs is too
    got = load(AC.write(tmp_path / "a.wav", samples, fmt, sr_in))
    assert got.shape == (32000,)
    err = np.abs(got - AC.reference(x, sr_in, 16000)).max()
    tol = AC.tolerance(table, half, np.abs(x).max())
    print(f"audio_load {case}: max|device - float64| = {err:.3e}, bound {tol:.3e}")
    assert err <= tol and (sr_in != 44100 or 4e-5 < tol < 7e-5)


def test_mel_of_the_example_audio(tmp_path):
    from s2v_amd import audio, inference
    wav = audio.load_audio(AUDIO_1, 16000, DEV)
    host = inference.load_wav(AUDIO_1, 16000)
    assert wav.shape == host.shape and wav.dtype == torch.float32
    mel = audio.melspectrogram(wav)
    ref = audio.melspectrogram(torch.from_numpy(host).to(DEV))
    assert mel.shape == ref.shape
    d = (mel - ref).abs().max().item()
    print(f"audio_load audio_1.wav: max|mel(device) - mel(host)| = {d:.3e}, "
          f"max|wav| = {(wav.cpu() - torch.from_numpy(host)).abs().max().item():.3e}")
    assert d <= 1e-3                                                       # the project's mel tolerance


# ----------------------------------------------------------------------------- CLI
def face_npy(tmp_path):
    rng = np.random.default_rng(3)
    p = tmp_path / "face.npy"
    np.save(p, rng.integers(0, 256, (4, 96, 128, 3), dtype=np.uint8))
    return str(p)


def test_run_device_equals_host_at_16k(tmp_path):
    from s2v_amd import inference
    face = face_npy(tmp_path)
    wav = AC.write(tmp_path / "a.wav", AC.random_codes("s16", 8000, 1, 9) // 4, "s16", 16000)
    host = inference.run(face, wav, max_frames=4)
    dev = inference.run(face, wav, max_frames=4, audio_load="device")
    assert host["meta"]["audio_load"] == "host" and dev["meta"]["audio_load"] == "device"
    assert dev["meta"]["frames"] == host["meta"]["frames"] == 4
    assert torch.equal(dev["preds"], host["preds"]) and torch.equal(dev["frames"], host["frames"])
    for key in ("mel_cols", "mel_windows", "wav_samples_16k"):
        assert dev["meta"][key] == host["meta"][key]


def test_run_modes_agree_on_the_example_audio(tmp_path, monkeypatch):
    from s2v_amd import inference
    face = face_npy(tmp_path)
    host = inference.run(face, AUDIO_1, max_frames=2)
    monkeypatch.setenv("S2V_AUDIO_LOAD", "device")
    dev = inference.run(face, AUDIO_1, max_frames=2, audio_load=None)
    assert dev["meta"]["audio_load"] == "device" and host["meta"]["audio_load"] == "host"
    for key in ("frames", "mel_cols", "mel_windows", "wav_samples_16k"):
        assert dev["meta"][key] == host["meta"][key]


def test_cli_reads_and_muxes_a_float_wav(tmp_path, capsys):
    from s2v_amd import audio, inference, mjpeg
    face = face_npy(tmp_path)
    t = np.arange(12000) / 24000.0
    x = np.stack([0.5 * np.sin(2 * np.pi * 440 * t), 1.2 * np.sin(2 * np.pi * 330 * t)], 1).astype(np.float32)
    wav = AC.write(tmp_path / "tts.wav", x, "f32", 24000)
    args = ["--face", face, "--audio", wav, "--max_frames", "4", "--outfile", str(tmp_path / "x.avi")]
    with pytest.raises(wave.Error):
        inference.main(args)                                               # the host path cannot open the file
    capsys.readouterr()
    assert inference.main(args + ["--audio_load", "device"]) == 0
    meta = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert meta["audio_load"] == "device" and meta["frames"] == 4 and meta["wav_samples_16k"] == 8000
    rd = mjpeg.AviReader(str(tmp_path / "x.avi"))
    pcm, rate = audio.pcm16(wav)
    assert rate == rd.audio_rate == 24000 and rd.channels == 2 and len(rd) == 4
    assert (pcm == np.clip(np.rint(x.astype(np.float64) * 32768), -32768, 32767)).all() and pcm.min() == -32768
    assert (rd.pcm == MC.pcm_reference(pcm, 24000, 4, rd.rate, rd.scale)).all() and len(rd.pcm) == 4 * 24000 // 25
