"""configs[0] runner host pieces (s2v_amd.inference): PCM .wav loading + resampling to 16 kHz
(librosa.load(sr=16000), futils/audio.py:10-11 — resampy's filter is absent: parity UNPINNED, the
checks are the properties a band-limited resampler must have) and the MP4 header reader that sizes
the synthetic frames."""
import os

import numpy as np

import s2v_import  # noqa: F401
from helpers import write_mp4_header, write_wav
from conftest import GOLDEN
from s2v_amd import inference

# the reference's examples/face/1.mp4 and examples/audio/1.wav, stored unchanged as fixtures
EXAMPLES = os.path.join(GOLDEN, "examples")


def test_load_wav_resamples_and_downmixes(tmp_path):
    p = write_wav(tmp_path / "a.wav", rate=44100, channels=2, seconds=1.0, freq=440.0, amp=0.5)
    x = inference.load_wav(str(p), 16000)
    assert x.dtype == np.float32 and len(x) == 16000
    mid = x[2000:14000]                                   # mono = mean of (s, s/2) = 0.75 s
    spec = np.abs(np.fft.rfft(mid * np.hanning(len(mid))))
    assert abs(np.argmax(spec) * 16000 / len(mid) - 440.0) < 2.0
    assert abs(np.abs(mid).max() - 0.375) < 0.375 * 0.01
    # a tone above the new Nyquist is removed
    q = write_wav(tmp_path / "b.wav", rate=44100, channels=1, seconds=0.5, freq=10000.0, amp=0.5)
    assert np.abs(inference.load_wav(str(q), 16000)[1000:-1000]).max() < 5e-3


def test_load_wav_at_16k_is_the_pcm(tmp_path):
    p = write_wav(tmp_path / "c.wav", rate=16000, channels=1, seconds=0.25)
    x = inference.load_wav(str(p), 16000)
    import wave
    with wave.open(str(p)) as w:
        pcm = np.frombuffer(w.readframes(w.getnframes()), "<i2")
    assert np.array_equal(x, pcm.astype(np.float32) / 32768.0)


def test_mp4_header_reader(tmp_path):
    p = write_mp4_header(tmp_path / "v.mp4", 700, 700, 135, 12800, 69120)
    info = inference.mp4_video_info(str(p))
    assert info["width"] == 700 and info["height"] == 700 and info["frames"] == 135
    assert abs(info["fps"] - 135 * 12800 / 69120) < 1e-9


def test_reference_examples_headers():
    info = inference.mp4_video_info(os.path.join(EXAMPLES, "face_1.mp4"))
    assert (info["width"], info["height"], info["frames"]) == (700, 700, 135)
    x = inference.load_wav(os.path.join(EXAMPLES, "audio_1.wav"), 16000)
    assert abs(len(x) / 16000 - 221184 / 44100) < 1e-3
