#!/usr/bin/env python3
"""Timing of the device JPEG encoder (mjpeg.JpegEncoder over s2v_jpeg_encode) on batches of 16 synthetic uint8
BGR frames, 700x700 and 1400x1400 (the CLI's plain and --enhance output of examples/face/1.mp4), quality 95.

    python tools/mjpeg_micro.py [--iters 20] [--batch 16] [--hw 700 700] [--out profiles/mjpeg_micro.txt]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o run -- \\
        python tools/mjpeg_micro.py --hw 1400 1400 --profile 20

Frames: a smooth picture (gradients, two sinusoids, a disc that moves from frame to frame) plus uniform noise
of +-12 grey levels per channel, from a fixed seed.  Per size, one JSON line:
  * ``encode_ms``: HIP events around JpegEncoder.encode (the three launches: transform, entropy, compact),
    median and min of --iters;
  * ``encode_to_host_ms``: wall clock of encode_to_host (launches + the sizes copy + the copy of the used bytes);
  * ``bytes_out`` / ``bytes_raw``, and the PSNR of the first and last stream, decoded by Pillow, against its frame;
  * ``host``: for comparison in the same session, the device -> host copy of the raw batch and Pillow's
    save(quality=95, subsampling=2) of the same frames, one after the other on one CPU thread.
``--profile N``: one warm batch, then N encode() calls per size and nothing else (for the kernel trace)."""
import argparse
import io
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import s2v_import  # noqa: E402,F401


def frames_of(n, h, w, seed=0):
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float32)
    out = np.empty((n, h, w, 3), np.uint8)
    for i in range(n):
        disc = ((x - w * (0.3 + 0.02 * i)) ** 2 + (y - h * 0.45) ** 2 < (0.18 * min(h, w)) ** 2).astype(np.float32)
        base = np.stack([110.0 + 90.0 * np.sin(x / (0.09 * w) + 0.3 * i) * np.cos(y / (0.13 * h)),
                         255.0 * (x + y) / (h + w), 60.0 + 120.0 * disc + 40.0 * np.sin(y / (0.05 * h))], axis=2)
        noise = rng.integers(-12, 13, (h, w, 3)).astype(np.float32)
        out[i] = np.clip(np.rint(base + noise), 0, 255).astype(np.uint8)
    return out


def median_min(ts):
    ts = sorted(ts)
    return {"median": round(ts[len(ts) // 2], 3), "min": round(ts[0], 3)}


def event_ms(fn, iters):
    ts = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    return median_min(ts)


def wall_ms(fn, iters):
    ts = []
    for _ in range(iters):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t) * 1e3)
    return median_min(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--quality", type=int, default=95)
    ap.add_argument("--host_iters", type=int, default=3)
    ap.add_argument("--profile", type=int, default=0)
    ap.add_argument("--hw", type=int, nargs=2, action="append", default=None, help="a frame size (default: both)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from PIL import Image

    from s2v_amd import mjpeg
    lines = []
    for h, w in (a.hw or ((700, 700), (1400, 1400))):
        host = frames_of(a.batch, h, w)
        dev = torch.from_numpy(host).cuda()
        enc = mjpeg.JpegEncoder(h, w, quality=a.quality, order="bgr")
        files = enc.encode_to_host(dev)
        torch.cuda.synchronize()
        if a.profile:
            for _ in range(a.profile):
                enc.encode(dev)
            torch.cuda.synchronize()
            lines.append(json.dumps({"hw": [h, w], "profiled_encodes": a.profile, "encodes_in_trace": a.profile + 1}))
            continue
        # the streams are pictures of the frames: Pillow decodes the first and the last
        psnr = []
        for i in (0, a.batch - 1):
            dec = np.array(Image.open(io.BytesIO(files[i])).convert("RGB"))[..., ::-1].astype(np.float64)
            psnr.append(round(float(10.0 * np.log10(255.0 ** 2 / ((dec - host[i]) ** 2).mean())), 2))
        assert min(psnr) > 30.0, psnr
        out = torch.empty((a.batch, enc.capacity), dtype=torch.uint8, device="cuda")
        enc_ms = event_ms(lambda: enc.encode(dev, out=out), a.iters)
        full_ms = wall_ms(lambda: enc.encode_to_host(dev), a.iters)
        d2h_ms = wall_ms(lambda: dev.cpu(), a.host_iters)

        def pillow():
            n = 0
            for f in host:
                bio = io.BytesIO()
                Image.fromarray(f[..., ::-1]).save(bio, "JPEG", quality=a.quality, subsampling=2)
                n += bio.tell()
            return n
        pil_bytes = pillow()
        pil_ms = wall_ms(pillow, a.host_iters)
        lines.append(json.dumps({
            "hw": [h, w], "batch": a.batch, "quality": a.quality, "iters": a.iters,
            "device": torch.cuda.get_device_name(0),
            "encode_ms": enc_ms, "encode_frames_per_s": round(a.batch / enc_ms["median"] * 1e3, 1),
            "encode_to_host_ms": full_ms, "encode_to_host_frames_per_s": round(a.batch / full_ms["median"] * 1e3, 1),
            "bytes_out": sum(len(f) for f in files), "bytes_raw": int(host.nbytes), "psnr_db_first_last": psnr,
            "workspace_bytes": int(enc._ws.numel()), "capacity_bytes": enc.capacity,
            "host": {"d2h_raw_ms": d2h_ms, "pillow_ms": pil_ms, "pillow_bytes": pil_bytes,
                     "frames_per_s": round(a.batch / (d2h_ms["median"] + pil_ms["median"]) * 1e3, 1)},
        }))
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
