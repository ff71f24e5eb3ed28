#!/usr/bin/env python3
"""FAN landmark path on the device (synthetic weights): launches per forward, frames/s of crop + network +
peaks at B faces in each conv precision, and the achieved fraction of HBM peak of the two elementwise
kernels on algorithmic bytes (HIP events around warm iterations, medians).

    python tools/fan_micro.py [--batch 16] [--iters 20] [--elt-batch 64]

Prints one JSON line per measurement.  The elementwise kernels run on [elt-batch, 64, 64, 256] tensors
(268 MB each at 64: past the 256 MB last-level cache, so the rate is HBM's), bytes = what the kernel must
read and write once; the peak is 8 TB/s.
"""
import argparse
import json
import os
import sys
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import s2v_import  # noqa: E402,F401

HBM_PEAK = 8e12


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
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--elt-batch", type=int, default=64)
    a = ap.parse_args()
    from s2v_amd import face_detection as fd, models, ops, synth
    from s2v_amd.engine import fan as fan_engine
    from s2v_amd.models.fan_arch import FANParams
    from s2v_amd.ops import NHWC
    dev = torch.device("cuda")
    name = torch.cuda.get_device_name(0)
    net = models.FAN()
    net.load_state_dict(synth.synth_torch_state_dict(FANParams(), **synth.FAN_SYNTH), strict=True)
    boxes_given = types.SimpleNamespace(reference_scale=195)            # the boxes are given: S3FD is not timed here
    fa = fd.FaceAlignment(fd.LandmarksType._2D, device=dev, detector=boxes_given, fan=net.eval())
    B = a.batch
    frames = torch.from_numpy(synth.sr_frame("fan.micro", B, 360, 480)).to(dev)
    boxes = [np.array([150.0 + 3 * i, 90.0 + 2 * i, 330.0 + 3 * i, 290.0 + 2 * i, 0.99], np.float32) for i in range(B)]
    cs = [fd.box_center_scale(b) for b in boxes]
    table = fd.crop_table(range(B), [c for c, _ in cs], [s for _, s in cs], (360, 480))

    def device_part():
        return fa.peaks(fa._fan(fa.crops(frames, table)))

    # launches of one warm forward, by kind
    device_part()
    counts = {}
    real = {k: getattr(fan_engine, k) for k in ("bn_act", "merge")}
    real_conv = fan_engine.ops.conv2d

    def counted(key, fn):
        def f(*args, **kw):
            counts[key] = counts.get(key, 0) + 1
            return fn(*args, **kw)
        return f
    fan_engine.bn_act, fan_engine.merge = counted("bn_act", real["bn_act"]), counted("merge", real["merge"])
    fan_engine.ops.conv2d = counted("conv2d", real_conv)
    try:
        device_part()
    finally:
        fan_engine.bn_act, fan_engine.merge, fan_engine.ops.conv2d = real["bn_act"], real["merge"], real_conv
    print(json.dumps({"launches_per_forward": sum(counts.values()), "by_kind": counts,
                      "budget": fan_engine.LAUNCH_BUDGET, "plus": "1 crop + 1 peaks per batch"}))

    for prec in ("f16x3", "bf16x3", "f32"):
        with ops.precision(prec):
            device_part()
            device_part()
            med, mn = event_ms(device_part, a.iters)
            full_med, _ = event_ms(lambda: fa.get_landmarks_from_batch(frames, detected_faces=[[b] for b in boxes]),
                                   max(3, a.iters // 4))
        print(json.dumps({"device": name, "precision": prec, "faces": B, "crop_network_peaks_ms": {
            "median": round(med, 3), "min": round(mn, 3)}, "frames_per_s": round(B / med * 1e3, 1),
            "with_host_tables_and_point_maps_ms": round(full_med, 3),
            "frames_per_s_with_host": round(B / full_med * 1e3, 1)}))

    # the two elementwise kernels on algorithmic bytes
    n, h, w, c = a.elt_batch, 64, 64, 256
    ctx = ops.Ctx(dev)
    x, b2 = NHWC(torch.randn(n, h, w, c, device=dev)), NHWC(torch.randn(n, h, w, c, device=dev))
    bn = (torch.rand(c, device=dev) + 0.5, torch.randn(c, device=dev))
    y = NHWC.empty(n, h, w, c, dev)
    elems = n * h * w * c
    cases = (("s2v_bn_act_nhwc", lambda: fan_engine.bn_act(ctx, x, bn, y), 2.0),
             ("s2v_fan_merge a+b -> s, relu(bn(s)), pool, relu(bn(pool))",
              lambda: fan_engine.merge(ctx, x, b2, bn_a=bn, pool=True, bn_b=bn), 2 + 2 + 0.5),
             ("s2v_fan_merge a+b -> s, relu(bn(s))", lambda: fan_engine.merge(ctx, x, b2, bn_a=bn), 4.0))
    reps = 10                       # launches per timed interval: the host's launch work hides behind the queue
    for label, fn, tensors in cases:
        fn()
        med, mn = (t / reps for t in event_ms(lambda: [fn() for _ in range(reps)], a.iters))
        nbytes = tensors * elems * 4
        print(json.dumps({"kernel": label, "shape": [n, h, w, c], "algorithmic_MB": round(nbytes / 1e6, 1),
                          "ms": {"median": round(med, 4), "min": round(mn, 4)},
                          "TB_per_s": round(nbytes / (med * 1e-3) / 1e12, 3),
                          "of_hbm_peak": round(nbytes / (med * 1e-3) / HBM_PEAK, 3)}))


if __name__ == "__main__":
    main()
