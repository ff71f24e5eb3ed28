#!/usr/bin/env python3
"""GANimation upper-face stage on the device (synthetic weights): launches per forward, the time of input build
+ generator + blend at B faces of 128 x 128 in each conv precision, the three kernels of csrc/gani.hip as launch
periods on their algorithmic bytes, the stage's share of the ENet step it follows, and the same network in torch
on the host CPU (HIP events around warm iterations, medians).

    python tools/ganimation_micro.py [--batch 16] [--iters 20] [--no-cpu]

Prints one JSON line per measurement.  A launch period is the time per launch of ``reps`` back-to-back launches
(the host's launch work hides behind the queue); bytes are what a kernel must read and write once.  The working
sets (7-40 MB) sit inside the 256 MB last-level cache, so the rates are not HBM's.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

import s2v_import  # noqa: E402,F401

ENET_STEP_MS = 23.7          # the flagship ENet(+LNet) step at batch 16 that the stage follows (README)


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


def torch_cpu_forward(sd, img, aus):
    """SplitGenerator.forward (model_utils.py:474-482) from the state_dict alone, in torch on the CPU."""
    def w(k):
        return sd[k + ".weight"], sd[k + ".bias"]
    x = torch.cat([img, aus[:, :, None, None].expand(-1, -1, *img.shape[2:])], 1)
    h = F.relu(F.instance_norm(F.conv2d(x, *w("model.0"), padding=3)))
    for i in (3, 6):
        h = F.relu(F.instance_norm(F.conv2d(h, *w(f"model.{i}"), stride=2, padding=1)))
    for i in range(9, 15):
        t = F.relu(F.instance_norm(F.conv2d(h, *w(f"model.{i}.conv_block.0"), padding=1)))
        h = h + F.instance_norm(F.conv2d(t, *w(f"model.{i}.conv_block.3"), padding=1))
    for i in (15, 18):
        h = F.relu(F.instance_norm(F.conv_transpose2d(h, *w(f"model.{i}"), stride=2, padding=1)))
    return (torch.tanh(F.conv2d(h, sd["color_top.0.weight"], padding=3)),
            torch.sigmoid(F.conv2d(h, sd["au_top.0.weight"], padding=3)), h)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--no-cpu", action="store_true", help="skip the torch-CPU forward")
    a = ap.parse_args()
    from s2v_amd import ganimation, models, ops, synth
    from s2v_amd.engine import ganimation as eng
    dev = torch.device("cuda", 0)
    name = torch.cuda.get_device_name(0)
    net = models.SplitGenerator()
    sd = synth.synth_torch_state_dict(net, **synth.GANIMATION_SYNTH)
    net.load_state_dict(sd, strict=True)
    model = ganimation.GANimationModel().initialize(net_gen=net.eval(), device=dev).setup()
    B, P, S = a.batch, 384, ganimation.FINAL_SIZE
    orig = torch.from_numpy(synth.sr_frame("ganimation.micro", B, P, P)).to(dev)
    aus = ganimation.exp_aus_dict["surprise"].repeat(B, 1).to(dev)
    pred = torch.rand((B, 3, P, P), device=dev) * 1.5 - 0.25
    out_u8 = torch.empty((B, 3, P, P), dtype=torch.uint8, device=dev)
    ctx = ops.Ctx(dev)

    # launches of one warm forward, by kind
    model.edit(orig, aus)
    counts = {}
    real_conv, real_norm = eng.ops.conv2d, eng.ops.instnorm
    real_under = ops._conv

    def counted(key, fn):
        def f(*args, **kw):
            counts[key] = counts.get(key, 0) + 1
            return fn(*args, **kw)
        return f
    ops._conv, eng.ops.instnorm = counted("conv launches", real_under), counted("instnorm", real_norm)
    try:
        model.edit(orig, aus)
    finally:
        ops._conv, eng.ops.instnorm = real_under, real_norm
    print(json.dumps({"launches_per_forward": sum(counts.values()), "by_kind": counts, "planned": eng.LAUNCHES,
                      "plus": "1 input build + 1 blend per batch, 1 composite in place of the uint8 conversion"}))

    stage = {}
    for prec in ("f16x3", "bf16x3", "f32"):
        with ops.precision(prec):
            model.edit(orig, aus)
            model.edit(orig, aus)
            med, mn = event_ms(lambda: model.edit(orig, aus), a.iters)
        stage[prec] = med
        print(json.dumps({"device": name, "precision": prec, "faces": B, "hw": [S, S],
                          "input_generator_blend_ms": {"median": round(med, 3), "min": round(mn, 3)},
                          "faces_per_s": round(B / med * 1e3, 1)}))

    # the three kernels on algorithmic bytes
    x20 = ganimation.gani_input(ctx, orig, aus)
    head = ops.NHWC(torch.randn((B, S, S, 4), device=dev))
    fake = torch.rand((B, 3, S, S), device=dev) * 2 - 1
    px, pp = B * S * S, B * P * P
    cases = (("s2v_gani_input 384 -> 128", lambda: ganimation.gani_input(ctx, orig, aus), pp * 3 + B * 17 * 4 + px * 80),
             ("s2v_gani_blend", lambda: net.blend(ctx, head, x20), px * (16 + 16 + 7 * 4)),
             ("s2v_gani_compose 128 -> 384, uint8 out", lambda: ganimation.gani_compose(ctx, pred, orig, fake, out_u8),
              pp * 3 * (4 + 1 + 1) + px * 3 * 4),
             ("s2v_gani_compose originals, uint8 out", lambda: ganimation.gani_compose(ctx, pred, orig, None, out_u8),
              pp * 3 * (4 + 1 + 1)),
             ("s2v_to_u8 (the conversion the composite replaces)",
              lambda: ops.S2V.to_u8_(pred, out_u8, 0.0, 1.0, 255.0, 0.0), pp * 3 * (4 + 1)))
    reps = 10
    periods = {}
    for label, fn, nbytes in cases:
        fn()
        med, mn = (t / reps for t in event_ms(lambda: [fn() for _ in range(reps)], a.iters))
        periods[label] = med
        print(json.dumps({"kernel": label, "faces": B, "algorithmic_MB": round(nbytes / 1e6, 2),
                          "launch_period_ms": {"median": round(med, 4), "min": round(mn, 4)},
                          "TB_per_s": round(nbytes / (med * 1e-3) / 1e12, 3)}))
    added = stage["f16x3"] + periods["s2v_gani_compose 128 -> 384, uint8 out"] - \
        periods["s2v_to_u8 (the conversion the composite replaces)"]
    print(json.dumps({"stage_added_to_a_batch_ms": round(added, 3), "precision": "f16x3", "enet_step_ms": ENET_STEP_MS,
                      "share_of_enet_step": round(added / ENET_STEP_MS, 4)}))

    if not a.no_cpu:
        torch.set_num_threads(min(16, os.cpu_count() or 1))
        img = torch.from_numpy(synth.hash_array("ganimation.micro.img", (B, 3, S, S), -1.0, 1.0))
        au = ganimation.exp_aus_dict["surprise"].repeat(B, 1)
        with torch.no_grad():
            torch_cpu_forward(sd, img, au)
            ts = []
            for _ in range(3):
                t0 = time.perf_counter()
                torch_cpu_forward(sd, img, au)
                ts.append(time.perf_counter() - t0)
        med = sorted(ts)[1]
        print(json.dumps({"cpu": "SplitGenerator layer for layer in torch CPU fp32 (host of the device)",
                          "threads": torch.get_num_threads(), "faces": B, "hw": [S, S],
                          "network_ms_median": round(med * 1e3, 1), "faces_per_s": round(B / med, 1),
                          "device_speedup_f16x3": round(med * 1e3 / stage["f16x3"], 1)}))


if __name__ == "__main__":
    main()
