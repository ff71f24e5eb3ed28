#!/usr/bin/env python3
"""Timing of the device JPEG decoder (mjpeg.JpegDecoder over s2v_jpeg_decode) on batches of 16 frames, 700x700 and
1400x1400 at quality 95 (the frames of tools/mjpeg_micro.py), from two kinds of stream:

  * ``own``: the project's encoder's streams: one restart interval per MCU row (44 or 88 intervals a frame);
  * ``pillow``: Pillow's default streams of the same frames: no restart markers, one interval a frame, so one lane
    decodes a whole frame.

    python tools/mjpeg_decode_micro.py [--iters 10] [--batch 16] [--hw 700 700] [--out profiles/mjpeg_decode_micro.txt]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o run -- \\
        python tools/mjpeg_decode_micro.py --hw 700 700 --streams own --split 0 --profile 10

Per size, stream kind and work split of the entropy kernel (``split`` 0: one wave per interval, 1: one lane), one
JSON line:
  * ``pack_ms``: the host's share, parse_jpeg + the marker scan + the one buffer (wall clock);
  * ``upload_ms``: the one host -> device copy of that buffer (wall clock, synchronised);
  * ``launch_ms``: HIP events around the launches (status clear, entropy, IDCT, upsample + colour);
  * ``decode_ms``: wall clock of JpegDecoder.decode, everything above, synchronised;
  * ``stream_gb_per_s`` / ``pixel_gb_per_s``: stream bytes in and RGB bytes out per second of ``launch_ms``, and
    ``hbm_fraction``: (stream + coefficients written and read + planes written and read + pixels) / launch time over
    the 8 TB/s of the part;
  * ``host``: the same files through Pillow, frame by frame on one CPU thread, plus the upload of the raw batch,
    in the same session; ``speedup_vs_host``: its time over ``decode_ms``.
The first frame of every configuration is compared with Pillow's pixels before anything is timed.
``--profile N``: one warm batch, then N decode_packed() calls of one configuration and nothing else."""
import argparse
import io
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import s2v_import  # noqa: E402,F401
from mjpeg_micro import event_ms, frames_of, wall_ms  # noqa: E402

HBM_BYTES_PER_S = 8.0e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--quality", type=int, default=95)
    ap.add_argument("--host_iters", type=int, default=2)
    ap.add_argument("--profile", type=int, default=0)
    ap.add_argument("--streams", nargs="+", default=["own", "pillow"], choices=["own", "pillow"])
    ap.add_argument("--split", type=int, nargs="+", default=[0, 1], choices=[0, 1])
    ap.add_argument("--hw", type=int, nargs=2, action="append", default=None, help="a frame size (default: both)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from PIL import Image

    from s2v_amd import mjpeg
    lines = []
    for h, w in (a.hw or ((700, 700), (1400, 1400))):
        host = frames_of(a.batch, h, w)
        for kind in a.streams:
            if kind == "own":
                files = mjpeg.JpegEncoder(h, w, quality=a.quality, order="bgr").encode_to_host(torch.from_numpy(host).cuda())
            else:
                files = []
                for f in host:
                    bio = io.BytesIO()
                    Image.fromarray(f[..., ::-1]).save(bio, "JPEG", quality=a.quality, subsampling=2)
                    files.append(bio.getvalue())
            ref0 = np.array(Image.open(io.BytesIO(files[0])).convert("RGB"))[..., ::-1]

            def pillow():
                return torch.from_numpy(np.stack([np.asarray(Image.open(io.BytesIO(f)).convert("RGB")) for f in files])).cuda()
            host_ms = None
            for split in a.split:
                dec = mjpeg.JpegDecoder(h, w, 2, order="bgr", split=split)
                out = torch.empty((a.batch, h, w, 3), dtype=torch.uint8, device="cuda")
                _, status = dec.decode(files, out=out)
                assert status.tolist() == [0] * a.batch and np.array_equal(out[0].cpu().numpy(), ref0)
                buf, offs, cnt = mjpeg.pack_streams(files, h, w, 2)
                dev = torch.from_numpy(buf).cuda()
                if a.profile:
                    for _ in range(a.profile):
                        dec.decode_packed(dev, offs, cnt, out)
                    torch.cuda.synchronize()
                    lines.append(json.dumps({"hw": [h, w], "streams": kind, "split": split, "profiled_decodes": a.profile,
                                             "decodes_in_trace": a.profile + 1}))
                    continue
                if host_ms is None:
                    host_ms = wall_ms(lambda: (pillow(), torch.cuda.synchronize()), a.host_iters)
                pack_ms = wall_ms(lambda: mjpeg.pack_streams(files, h, w, 2), a.iters)
                upload_ms = wall_ms(lambda: (torch.from_numpy(buf).cuda(), torch.cuda.synchronize()), a.iters)
                launch_ms = event_ms(lambda: dec.decode_packed(dev, offs, cnt, out), a.iters)
                decode_ms = wall_ms(lambda: (dec.decode(files, out=out), torch.cuda.synchronize()), a.iters)
                sec = launch_ms["median"] * 1e-3
                stream_bytes, pixel_bytes = cnt["data_bytes"], a.batch * h * w * 3
                ws = int(dec._ws.numel())
                lines.append(json.dumps({
                    "hw": [h, w], "batch": a.batch, "quality": a.quality, "iters": a.iters, "streams": kind,
                    "split": ("wave", "lane")[split], "device": torch.cuda.get_device_name(0),
                    "intervals": cnt["intervals"], "stream_bytes": stream_bytes, "pixel_bytes": pixel_bytes,
                    "workspace_bytes": ws, "pack_ms": pack_ms, "upload_ms": upload_ms, "launch_ms": launch_ms,
                    "decode_ms": decode_ms, "decode_frames_per_s": round(a.batch / decode_ms["median"] * 1e3, 1),
                    "stream_gb_per_s": round(stream_bytes / sec / 1e9, 3), "pixel_gb_per_s": round(pixel_bytes / sec / 1e9, 2),
                    "hbm_fraction": round((stream_bytes + 2 * ws + pixel_bytes) / sec / HBM_BYTES_PER_S, 4),
                    "host": {"pillow_decode_and_upload_ms": host_ms,
                             "frames_per_s": round(a.batch / host_ms["median"] * 1e3, 1)},
                    "speedup_vs_host": round(host_ms["median"] / decode_ms["median"], 2),
                }))
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
