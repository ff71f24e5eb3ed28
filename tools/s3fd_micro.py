#!/usr/bin/env python3
"""Timing of face_detection.SFDDetector.detect_from_batch (S3FD, synthetic weights) on a batch of
synthetic uint8 frames: HIP events around warm iterations, default conv precision.

    python tools/s3fd_micro.py [--batch 4 --h 700 --w 700] [--iters 20] [--nms host|device]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o run -- python tools/s3fd_micro.py --profile 5

``--profile N``: one calibrating + one warm batch, then N batches and nothing else (divide the
trace's per-kernel calls by N + 2).  Prints one JSON line.  Random weights pass a few percent of the
positions, so the host NMS handles more rows than a real frame gives; ``network_ms`` (input prep + S3FD +
decode + the one device -> host copy, no NMS) stands beside the full call.  ``--nms device``: the full call
with SFDDetector(nms="device") (s2v_nms, only the kept rows copied); ``nms_status`` lists the kernel's status
per image (an image whose status is not 0 took the host path)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import s2v_import  # noqa: E402,F401


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--h", type=int, default=700)
    ap.add_argument("--w", type=int, default=700)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--profile", type=int, default=0)
    ap.add_argument("--nms", default="host", choices=["host", "device"])
    a = ap.parse_args()
    from s2v_amd import face_detection, models, ops, synth
    from s2v_amd.models.s3fd_arch import S3FDParams, level_sizes
    net = models.S3FD()
    net.load_state_dict(synth.s3fd_state_dict(S3FDParams()), strict=True)
    det = face_detection.SFDDetector("cuda", net=net.eval(), nms=a.nms)
    frames = torch.from_numpy(synth.sr_frame("s3fd.micro", a.batch, a.h, a.w)).cuda()
    dets = det.detect_from_batch(frames)                      # builds the engine, calibrates the range guard
    det.detect_from_batch(frames)
    torch.cuda.synchronize()
    if a.profile:
        for _ in range(a.profile):
            det.detect_from_batch(frames)
        torch.cuda.synchronize()
        print(json.dumps({"profiled_batches": a.profile, "batches_in_trace": a.profile + 2}))
        return
    cands = det.candidates(det.head_maps(frames))
    full_med, full_min = event_ms(lambda: det.detect_from_batch(frames), a.iters)
    net_med, net_min = event_ms(lambda: det.candidates(det.head_maps(frames)), a.iters)
    lv = level_sizes(a.h, a.w)
    extra = {}
    if a.nms == "device":
        from s2v_amd import face
        cand, count, n, P = det.decode(det.head_maps(frames))
        res = face.nms_device(cand, count, n, P, 8, face_detection.NMS_THRESH, min_score=face_detection.KEEP_THRESH,
                              keep_max=det.keep_max)
        extra = {"nms_status": [st for _, st in res], "keep_max": det.keep_max}
    print(json.dumps({
        "nms": a.nms, **extra,
        "batch": a.batch, "hw": [a.h, a.w], "precision": ops.PRECISION, "iters": a.iters,
        "device": torch.cuda.get_device_name(0),
        "detect_from_batch_ms": {"median": round(full_med, 3), "min": round(full_min, 3)},
        "frames_per_s": round(a.batch / full_med * 1e3, 1),
        "network_ms": {"median": round(net_med, 3), "min": round(net_min, 3)},
        "network_frames_per_s": round(a.batch / net_med * 1e3, 1),
        "levels": lv, "candidates_per_image": [len(c) for c in cands], "kept_per_image": [len(d) for d in dets],
    }))


if __name__ == "__main__":
    main()
