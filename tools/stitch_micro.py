#!/usr/bin/env python3
"""The reference stitch (s2v_amd.stitch) on the device: the launch period of its two launches for B frames of
256 x 256 (HIP events around ``reps`` back-to-back warm launches, divided by reps, medians), their rate on
algorithmic bytes, the host-side coefficient time per batch, and the same frames through Pillow on the host CPU
as the baseline.  A launch period includes the launch overhead between two kernels of the queue: at this size it
is an upper bound on the kernel's time, and the rates derived from it are lower bounds on the kernel's rate (a
kernel time proper comes from a kernel trace).

    python tools/stitch_micro.py [--batch 16] [--iters 20] [--reps 200]

Prints one JSON line per measurement.  Algorithmic bytes = what a launch must read and write once:
s2v_pil_transform_quad reads each frame's crop box and writes the crop; s2v_pil_perspective_paste reads crop and
target and writes the output.  At B = 16 that is ~3 MB per launch, which stays in the 256 MB last-level cache:
the share of the 8 TB/s HBM peak is reported as DESIGN 5a does for every kernel, and says how far such a small
launch is from a bandwidth-bound one, not that HBM is the limit.  The Pillow baseline runs wherever Pillow
imports; without it the line says so.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import s2v_import  # noqa: E402,F401

HBM_PEAK = 8e12
SIZE = 256


def event_ms(fn, iters):
    ts = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    ts.sort()
    return ts[len(ts) // 2], ts[0]


def quads_for(B):
    """Rotated squares as crop_faces builds them for faces of ~150 px that drift and turn."""
    out = []
    for i in range(B):
        t = np.deg2rad(-8.0 + 1.1 * i)
        c = np.array([128.0 + 1.5 * i, 131.0 - 0.7 * i])
        x = (118.0 + 0.9 * i) * np.array([np.cos(t), np.sin(t)])
        y = np.flipud(x) * [-1, 1]
        out.append(np.stack([c - x - y, c - x + y, c + x + y, c + x - y]))
    return out


def pillow_baseline(frames, bases, quads, iters):
    try:
        from PIL import Image
    except ImportError:
        return {"pillow": "not installed: no host baseline on this machine"}
    from s2v_amd import stitch as ST
    ts = []
    for _ in range(iters):
        t0 = time.perf_counter()
        for f, b, q in zip(frames, bases, quads):
            box, rel = ST.crop_box(q, SIZE, SIZE, SIZE)
            crop = Image.fromarray(f).crop(box).transform((SIZE, SIZE), Image.QUAD, (rel + 0.5).flatten(),
                                                          Image.BILINEAR)
            inv = ST.calc_alignment_coefficients(q + 0.5, ST.square(SIZE))
            pasted = Image.fromarray(b).convert("RGBA")
            proj = crop.convert("RGBA").transform((SIZE, SIZE), Image.PERSPECTIVE, inv, Image.BILINEAR)
            pasted.paste(proj, (0, 0), mask=proj)
            np.array(pasted.convert("RGB"))
        ts.append((time.perf_counter() - t0) * 1e3)
    ts.sort()
    import PIL
    return {"pillow": PIL.__version__, "host_cpu_ms_per_batch": {"median": round(ts[len(ts) // 2], 3),
                                                                 "min": round(ts[0], 3)}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--reps", type=int, default=200)
    a = ap.parse_args()
    from s2v_amd import post, stitch as ST, synth
    from s2v_amd._lib import check
    dev = torch.device("cuda")
    name = torch.cuda.get_device_name(0)
    B = a.batch
    frames_np = synth.sr_frame("stitch.micro.ref", B, SIZE, SIZE)
    bases_np = synth.sr_frame("stitch.micro.base", B, SIZE, SIZE)
    frames, bases = torch.from_numpy(frames_np).to(dev), torch.from_numpy(bases_np).to(dev)
    quads = quads_for(B)

    # host: the coefficient work of one batch (crop boxes, QUAD coefficients, the 8 x 8 solves)
    ts = []
    for _ in range(max(a.iters, 20)):
        t0 = time.perf_counter()
        table, boxes = ST.quad_table(quads, SIZE, SIZE, SIZE)
        inv = np.stack([ST.calc_alignment_coefficients(q + 0.5, ST.square(SIZE)) for q in quads])
        ts.append((time.perf_counter() - t0) * 1e3)
    ts.sort()
    print(json.dumps({"host_coefficients_ms_per_batch": {"median": round(ts[len(ts) // 2], 3), "min": round(ts[0], 3)},
                      "frames": B}))

    ctx = post._ctx(dev)
    tab, itab = torch.from_numpy(table).to(dev), torch.from_numpy(inv).to(dev)
    crops = torch.empty((B, SIZE, SIZE, 3), dtype=torch.uint8, device=dev)
    out = torch.empty((B, SIZE, SIZE, 3), dtype=torch.uint8, device=dev)
    img = SIZE * SIZE * 3
    row = SIZE * 3

    def quad():
        check(ctx.lib.s2v_pil_transform_quad(frames.data_ptr(), B, SIZE, SIZE, 3, row, img, tab.data_ptr(),
                                             crops.data_ptr(), SIZE, SIZE, row, img, ctx.stream), "quad")

    def paste():
        check(ctx.lib.s2v_pil_perspective_paste(crops.data_ptr(), B, SIZE, SIZE, 3, row, img, itab.data_ptr(),
                                                bases.data_ptr(), SIZE, SIZE, 3, row, img, out.data_ptr(), 3, row, img,
                                                ctx.stream), "paste")

    box_bytes = sum((b[2] - b[0]) * (b[3] - b[1]) * 3 for b in boxes)
    cases = (("s2v_pil_transform_quad", quad, box_bytes + B * img),
             ("s2v_pil_perspective_paste", paste, 3 * B * img))
    total = 0.0
    for label, fn, nbytes in cases:
        for _ in range(3):
            fn()
        med, mn = (t / a.reps for t in event_ms(lambda: [fn() for _ in range(a.reps)], a.iters))
        total += med
        print(json.dumps({"device": name, "kernel": label, "frames": B, "algorithmic_MB": round(nbytes / 1e6, 3),
                          "launch_period_us": {"median": round(med * 1e3, 2), "min": round(mn * 1e3, 2)},
                          "launches_per_interval": a.reps,
                          "TB_per_s_at_least": round(nbytes / (med * 1e-3) / 1e12, 3),
                          "of_hbm_peak_at_least": round(nbytes / (med * 1e-3) / HBM_PEAK, 4)}))

    # the whole stage as Stitcher runs it after the landmarks: host coefficients, two table uploads, two launches
    def stage():
        c, _ = ST.crop_faces_by_quads(SIZE, (None, frames), quads)
        cf = np.stack([ST.calc_alignment_coefficients(q + 0.5, ST.square(SIZE)) for q in quads])
        return ST.paste_images(cf, c, bases)

    stage()
    ts = []
    for _ in range(a.iters):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        stage()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    ts.sort()
    print(json.dumps({"stage_after_landmarks_ms_per_batch": {"median": round(ts[len(ts) // 2], 3), "min": round(ts[0], 3)},
                      "two_launch_periods_us": round(total * 1e3, 2), "frames": B}))
    ref = stage().cpu().numpy()
    base = pillow_baseline(frames_np, bases_np, quads, max(3, a.iters // 4))
    print(json.dumps(dict(base, frames=B)))
    if "pillow" in base and "host_cpu_ms_per_batch" in base:      # and the device result is Pillow's
        from PIL import Image
        q = quads[B // 2]
        box, rel = ST.crop_box(q, SIZE, SIZE, SIZE)
        crop = Image.fromarray(frames_np[B // 2]).crop(box).transform((SIZE, SIZE), Image.QUAD, (rel + 0.5).flatten(),
                                                                      Image.BILINEAR)
        pasted = Image.fromarray(bases_np[B // 2]).convert("RGBA")
        proj = crop.convert("RGBA").transform((SIZE, SIZE), Image.PERSPECTIVE,
                                              ST.calc_alignment_coefficients(q + 0.5, ST.square(SIZE)), Image.BILINEAR)
        pasted.paste(proj, (0, 0), mask=proj)
        print(json.dumps({"device_equals_pillow_on_frame": B // 2,
                          "equal": bool(np.array_equal(np.array(pasted.convert("RGB")), ref[B // 2]))}))


if __name__ == "__main__":
    main()
