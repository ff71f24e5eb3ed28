#!/usr/bin/env python3
"""Timing of the device audio loader (s2v_amd.audio.load_audio over s2v_audio_load) against the host route
(inference.load_wav + upload) on clips of the ``pipeline`` workload's length (40 s = 1000 frames at 25 fps):
44.1 kHz stereo s16 (the project's example audio's format), 48 kHz mono s16 and 22.05 kHz mono float32.

    python tools/audio_micro.py [--seconds 40] [--iters 10] [--out profiles/audio_micro.txt]

Per clip one JSON line:
  * ``host_ms``: inference.load_wav (stdlib ``wave`` + NumPy, float64 gather + einsum) and the upload of its float32
    result, wall clock, synchronised (the float32 file, which ``wave`` cannot open, is decoded with np.frombuffer and
    resampled with inference.resample: the host route such a file would have);
  * ``device_ms``: load_audio end to end: file read, header walk, one upload of the sample bytes, one launch, wall
    clock, synchronised; ``speedup_vs_host``: host_ms over it;
  * ``launch_ms``: the launch alone, HIP events around ``--reps`` back-to-back launches on resident bytes, per launch,
    after a warm launch;
  * what the kernel algorithmically moves: ``hbm_bytes`` (sample bytes in, float32 out, the table once) and
    ``table_bytes`` (2 half taps x 4 bytes per output, served by L1 / L2; the staged input is read as often from LDS),
    their rates over ``launch_ms`` and those rates over the part's 8 TB/s (HBM) and 34.5 TB/s (aggregate L2);
  * ``max_abs_err``: max |device - float64| over the whole clip, the reference evaluated directly from the formula
    (tests/audio_cases.py), and ``bound``, the derived fp32 bound of tests/test_audio_load_gpu.py.
The device result is compared with the host's before anything is timed."""
import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import audio_cases as AC  # noqa: E402
import s2v_import  # noqa: E402,F401
from mjpeg_micro import event_ms, wall_ms  # noqa: E402

HBM_BYTES_PER_S = 8.0e12
L2_BYTES_PER_S = 34.5e12
CLIPS = (("s16", 44100, 2), ("s16", 48000, 1), ("f32", 22050, 1))


def clip(fmt, rate, channels, seconds):
    """a voice-like seeded signal: a few drifting harmonics plus noise, 0.7 of full scale"""
    rng = np.random.default_rng(rate + channels)
    t = np.arange(int(rate * seconds)) / rate
    x = sum(a * np.sin(2 * np.pi * f * t * (1 + 0.01 * np.sin(2 * np.pi * 0.3 * t)))
            for a, f in ((0.3, 140.0), (0.2, 280.0), (0.1, 1210.0), (0.05, 3400.0)))
    x = np.stack([x + 0.05 * rng.standard_normal(len(t)) for _ in range(channels)], 1)
    x *= 0.7 / np.abs(x).max()
    return np.round(x * 32767).astype(np.int64) if fmt == "s16" else x.astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=40.0)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--host_iters", type=int, default=2)
    ap.add_argument("--reps", type=int, default=50, help="launches between one pair of events")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from s2v_amd import audio, inference, ops
    if not torch.cuda.is_available():
        raise SystemExit("audio_micro: no HIP device (there is no CPU path to time)")
    lines = []
    tmp = tempfile.mkdtemp(prefix="audio_micro")
    for fmt, rate, channels in CLIPS:
        samples = clip(fmt, rate, channels, a.seconds)
        path = AC.write(os.path.join(tmp, f"{fmt}_{rate}_{channels}.wav"), samples, fmt, rate)

        def host():
            if fmt == "f32":
                with open(path, "rb") as f:
                    raw = f.read()[44:]
                wav = inference.resample(np.frombuffer(raw, "<f4").reshape(-1, channels).mean(axis=1), rate, 16000)
            else:
                wav = inference.load_wav(path, 16000)
            return torch.from_numpy(wav).cuda()

        def device():
            return audio.load_audio(path, 16000, "cuda")
        got, ref = device(), host()                                   # warm (table built and uploaded), and checked
        torch.cuda.synchronize()
        x64 = AC.decode(samples, fmt).astype(np.float64).mean(axis=1)
        exact = AC.reference(x64, rate, 16000)
        table, up, down, half = audio.resample_table(rate, 16000)
        err = float(np.abs(got.cpu().numpy().astype(np.float64) - exact).max())
        bound = AC.tolerance(table, half, np.abs(x64).max())
        assert got.shape == ref.shape and err <= bound, (got.shape, ref.shape, err, bound)
        raw, _, _, kind, n_frames = audio.read_wav(path)
        pcm = torch.frombuffer(raw, dtype=torch.uint8).cuda()
        dtab = audio._device_table(rate, 16000, torch.device("cuda"))[0]
        out = torch.empty_like(got)

        def launches():
            for _ in range(a.reps):
                ops.S2V.audio_load_(pcm, n_frames, channels, kind, dtab, up, down, half, out)
        launches()
        torch.cuda.synchronize()
        assert torch.equal(out, got)
        launch = {k: round(v / a.reps, 5) for k, v in event_ms(launches, a.iters).items()}
        device_ms = wall_ms(lambda: (device(), torch.cuda.synchronize()), a.iters)
        host_ms = wall_ms(lambda: (host(), torch.cuda.synchronize()), a.host_iters)
        sec = launch["median"] * 1e-3
        hbm_bytes = len(raw) + 4 * out.numel() + 4 * table.size
        table_bytes = 4 * 2 * half * out.numel()
        lines.append(json.dumps({
            "clip": f"{a.seconds:g} s {rate} Hz {channels} ch {fmt}", "device": torch.cuda.get_device_name(0),
            "iters": a.iters, "host_iters": a.host_iters, "reps": a.reps, "frames_in": n_frames,
            "samples_out": out.numel(), "up": up, "down": down, "taps": 2 * half, "host_ms": host_ms,
            "device_ms": device_ms, "speedup_vs_host": round(host_ms["median"] / device_ms["median"], 1),
            "launch_ms": launch, "hbm_bytes": hbm_bytes, "hbm_gb_per_s": round(hbm_bytes / sec / 1e9, 1),
            "hbm_fraction": round(hbm_bytes / sec / HBM_BYTES_PER_S, 4), "table_bytes": table_bytes,
            "table_tb_per_s": round(table_bytes / sec / 1e12, 2),
            "l2_fraction": round(table_bytes / sec / L2_BYTES_PER_S, 3),
            "gfma_per_s": round(2 * half * out.numel() / sec / 1e9, 1),
            "max_abs_err": err, "bound": bound,
            "max_abs_device_minus_host": float((got - ref).abs().max().item()),
        }))
        print(lines[-1], flush=True)
        os.remove(path)
    os.rmdir(tmp)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    t0 = time.time()
    main()
    print(f"audio_micro: {time.time() - t0:.1f} s", file=sys.stderr)
