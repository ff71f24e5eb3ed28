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
``--profile N``: one warm batch, then N decode_packed() calls of one configuration and nothing else.

``--sync`` (profiles/mjpeg_sync_micro.txt) writes the rows of the sync split (s2v_jpeg_decode_sync) instead, all in
one session: per size and stream kind ``launch_ms`` and ``decode_ms`` (as above) of wave and of sync at every
``--sub_bytes``, the host route, the
longest interval and what ``auto`` picks, and for the streams without restart markers the resolving rounds per frame
(tools/jpeg_sync_host.cpp, compiled without sanitizers, on the same files); then ``crossover`` rows, wave against sync
at the default sub_bytes on Pillow's streams of small frames, from which SYNC_AUTO_BYTES is read."""
import argparse
import io
import json
import os
import shutil
import struct
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import s2v_import  # noqa: E402,F401
from mjpeg_micro import event_ms, frames_of, wall_ms  # noqa: E402

HBM_BYTES_PER_S = 8.0e12


def pillow_files(host, quality):
    from PIL import Image
    files = []
    for f in host:
        bio = io.BytesIO()
        Image.fromarray(f[..., ::-1]).save(bio, "JPEG", quality=quality, subsampling=2)
        files.append(bio.getvalue())
    return files


def host_rounds(files, h, w, sub, tmp):
    """resolving rounds of every interval at ``sub`` bytes a subsequence: tools/jpeg_sync_host.cpp on the CPU"""
    from s2v_amd import mjpeg
    exe = os.path.join(tmp, "jpeg_sync_host")
    if not os.path.exists(exe):
        cxx = next(p for p in (shutil.which(n) for n in ("c++", "g++", "clang++")) if p)
        subprocess.run([cxx, "-std=c++17", "-O2", os.path.join(ROOT, "tools", "jpeg_sync_host.cpp"), "-o", exe], check=True)
    buf, offs, cnt = mjpeg.pack_streams(files, h, w, 2)
    head = struct.pack("<16i", 0x4A563253, cnt["n"], h, w, 2, cnt["intervals"], cnt["max_per_frame"], cnt["sets"],
                       offs["intervals"], offs["frame_first"], offs["set_index"], offs["qtables"], offs["huff_sets"],
                       cnt["data_bytes"], 0, 0)
    with open(os.path.join(tmp, "tables.bin"), "wb") as f:
        f.write(head + buf[:offs["data"]].tobytes())
    names = []
    for k, data in enumerate(files):
        names.append(os.path.join(tmp, f"{k}.jpg"))
        with open(names[-1], "wb") as f:
            f.write(data)
    r = subprocess.run([exe, os.path.join(tmp, "tables.bin"), str(sub)] + names, capture_output=True, text=True, check=True)
    return [int(line.split()[2]) for line in r.stdout.splitlines() if line.startswith("rounds")]


def sync_rows(a):
    from PIL import Image

    from s2v_amd import mjpeg
    lines = []
    tmp = tempfile.mkdtemp(prefix="mjpeg_sync_micro")

    def launch(files, h, w, split, sub=None):
        dec = mjpeg.JpegDecoder(h, w, 2, order="bgr", split=split, sub_bytes=sub)
        out = torch.empty((len(files), h, w, 3), dtype=torch.uint8, device="cuda")
        _, status = dec.decode(files, out=out)                       # warm, and checked before anything is timed
        ref0 = np.array(Image.open(io.BytesIO(files[0])).convert("RGB"))[..., ::-1]
        assert status.tolist() == [0] * len(files) and np.array_equal(out[0].cpu().numpy(), ref0)
        buf, offs, cnt = mjpeg.pack_streams(files, h, w, 2)
        dev = torch.from_numpy(buf).cuda()
        ms = event_ms(lambda: dec.decode_packed(dev, offs, cnt, out), a.iters)
        dec.decode_ms = wall_ms(lambda: (dec.decode(files, out=out), torch.cuda.synchronize()), a.iters)
        return ms, cnt, dec

    for h, w in (a.hw or ((700, 700), (1400, 1400))):
        host = frames_of(a.batch, h, w)
        for kind in a.streams:
            if kind == "own":
                files = mjpeg.JpegEncoder(h, w, quality=a.quality, order="bgr").encode_to_host(torch.from_numpy(host).cuda())
            else:
                files = pillow_files(host, a.quality)

            def pillow():
                return torch.from_numpy(np.stack([np.asarray(Image.open(io.BytesIO(f)).convert("RGB")) for f in files])).cuda()
            wave, cnt, wdec = launch(files, h, w, "wave")
            _, _, auto = launch(files, h, w, "auto")
            row = {"hw": [h, w], "batch": a.batch, "quality": a.quality, "iters": a.iters, "streams": kind,
                   "device": torch.cuda.get_device_name(0), "intervals": cnt["intervals"],
                   "stream_bytes": cnt["data_bytes"], "longest_interval_bytes": cnt["max_interval_bytes"],
                   "auto_picks": auto.picked, "wave_launch_ms": wave, "wave_decode_ms": wdec.decode_ms,
                   "host_pillow_decode_and_upload_ms": wall_ms(lambda: (pillow(), torch.cuda.synchronize()), a.iters),
                   "sync": []}
            for sub in a.sub_bytes:
                ms, _, dec = launch(files, h, w, "sync", sub)
                entry = {"sub_bytes": sub, "launch_ms": ms, "decode_ms": dec.decode_ms, "workspace_bytes": int(dec._ws.numel()),
                         "wave_over_sync": round(wave["median"] / ms["median"], 2)}
                if kind == "pillow":
                    rounds = host_rounds(files, h, w, sub, tmp)
                    entry["rounds_per_frame"] = {"min": min(rounds), "median": sorted(rounds)[len(rounds) // 2],
                                                 "max": max(rounds)}
                row["sync"].append(entry)
            lines.append(json.dumps(row))
    for side in a.crossover:
        files = pillow_files(frames_of(a.batch, side, side), a.quality)
        wave, cnt, _ = launch(files, side, side, "wave")
        sync, _, _ = launch(files, side, side, "sync")
        lines.append(json.dumps({"crossover": [side, side], "batch": a.batch, "streams": "pillow",
                                 "longest_interval_bytes": cnt["max_interval_bytes"], "sub_bytes": mjpeg.SYNC_SUB_BYTES,
                                 "wave_launch_ms": wave, "sync_launch_ms": sync,
                                 "wave_over_sync": round(wave["median"] / sync["median"], 2)}))
    shutil.rmtree(tmp, ignore_errors=True)
    return lines


def write_lines(lines, out):
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            f.write(text)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sync", action="store_true", help="the rows of the sync split (profiles/mjpeg_sync_micro.txt)")
    ap.add_argument("--sub_bytes", type=int, nargs="+", default=[64, 128, 256, 512, 1024, 2048])
    ap.add_argument("--crossover", type=int, nargs="*", default=[32, 48, 64, 96, 128, 192, 256, 384],
                    help="with --sync: square frame sizes of the wave-against-sync rows")
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
    if a.sync:
        return write_lines(sync_rows(a), a.out)
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
    write_lines(lines, a.out)


if __name__ == "__main__":
    main()
