#!/usr/bin/env python3
"""Speed and error of the opt-in single-pass f16 conv arithmetic ("f16") against the default f16x3, on one box:

    python tools/f16_micro.py --time     > profiles/f16_micro.txt          # HIP-graph replays, HIP events
    python tools/f16_micro.py --precision profiles/f16_precision.json      # device error against the goldens
    python tools/f16_micro.py --emulate profiles/f16_precision.json        # CPU only: the mode on the reference math

``--time``: every shape / forward is captured once per mode into a HIP graph (device time only, no launch
overhead), warmed, then timed as ``--pairs`` interleaved (f16x3, f16) replay pairs; one JSON line each with the
medians, the median of the per-pair ratios f16 / f16x3 and the spread of the pairs (min / max ratio, and the
f16x3 replays' own max / min).  The forwards also report the share of their conv FLOPs that ran with prec 3
(ops.CONV_HOOK; the rest ran a fallback family as f16x3 or an exact-fp32 kernel).
``--precision`` / ``--emulate`` fill the "device" / "emulation" sections of the JSON: (max, mean) |difference| per
model output against the reference goldens (tests/golden) resp. of the CPU oracle with every conv operand rounded to
11 bits against the plain oracle (tests/f16_cases.py)."""
import argparse
import json
import os
import socket
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import s2v_import  # noqa: E402,F401

MODES = ("f16x3", "f16")


def box():
    p = torch.cuda.get_device_properties(0)
    return {"device": torch.cuda.get_device_name(0), "arch": getattr(p, "gcnArchName", ""), "cus": p.multi_processor_count,
            "host": socket.gethostname(), "torch": torch.__version__}


def capture(fn, reps):
    """``reps`` calls of fn() as one HIP graph (eager warm-up first: calibration, split weights, workspaces)."""
    st = torch.cuda.Stream()
    st.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(st):
        fn()
        fn()
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=st):
            for _ in range(reps):
                fn()
    torch.cuda.current_stream().wait_stream(st)
    g.replay()
    torch.cuda.synchronize()
    return g


def replay_ms(g, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    g.replay()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def pairs(name, fns, reps, npairs, extra=None):
    """fns: {mode: callable}, each captured under its mode; interleaved replays."""
    from s2v_amd import ops
    graphs = {}
    for m in MODES:
        with ops.precision(m):
            graphs[m] = capture(fns[m], reps)
    for m in MODES:                                          # warm both once more, interleaved
        replay_ms(graphs[m], reps)
    t = {m: [] for m in MODES}
    for _ in range(npairs):
        for m in MODES:
            t[m].append(replay_ms(graphs[m], reps))
    ratio = [b / a for a, b in zip(t["f16x3"], t["f16"])]
    rec = {"what": name, "pairs": npairs, "reps_per_replay": reps,
           "f16x3_ms": round(float(np.median(t["f16x3"])), 4), "f16_ms": round(float(np.median(t["f16"])), 4),
           "ratio_median": round(float(np.median(ratio)), 4), "ratio_min": round(min(ratio), 4),
           "ratio_max": round(max(ratio), 4),
           "f16x3_spread": round(max(t["f16x3"]) / min(t["f16x3"]), 4), "f16_spread": round(max(t["f16"]) / min(t["f16"]), 4)}
    rec.update(extra or {})
    print(json.dumps(rec), flush=True)
    return rec


def conv_case(ctx, n, h, w, cin, cout, modulated=False):
    """-> ({mode: launch}, {mode: symbol}, flops) of a 3x3 stride-1 conv; ``modulated``: per-sample weights."""
    from s2v_amd import ops
    from s2v_amd.ops import NHWC, ConvW
    g = torch.Generator().manual_seed(1)
    cw = ConvW(torch.randn(cout, cin, 3, 3, generator=g) / (3 * cin ** 0.5), torch.zeros(cout), "cuda", padding=1)
    x = NHWC(torch.rand((n, h, w, cin), device="cuda") * 2 - 1)
    y = NHWC.empty(n, h, w, cout, "cuda")
    s = torch.rand((n, cin), device="cuda") + 0.5
    d = torch.rand((n, cout), device="cuda") + 0.5

    def go():
        if modulated:
            ops.modulated_conv2d(ctx, x, cw, y, s, d, act=ops.ACT_LRELU, alpha=0.2)
        else:
            ops.conv2d(ctx, x, cw, y, act=ops.ACT_LRELU, alpha=0.2)
    syms = {}
    for m in MODES:
        seen = []

        def hook(c, p, flops, launch):
            seen.append(p.plan)
            launch()
        with ops.precision(m):
            go()                                             # calibrates the range guard
            ops.CONV_HOOK = hook
            try:
                go()
            finally:
                ops.CONV_HOOK = None
        syms[m] = [ops.plan_symbol(p) + (f" x{p[5]} splits" if p[5] > 1 else "") for p in seen]
    return {m: go for m in MODES}, syms, 2.0 * n * h * w * 9 * cin * cout


def time_convs(a):
    from s2v_amd import ops
    ctx = ops.Ctx("cuda")
    shapes = [("StyleConv 16x200^2 256->256 3x3 (256x256 tile)", (16, 200, 200, 256, 256), False),
              ("StyleConv 16x400^2 128->128 3x3 per-sample weights", (16, 400, 400, 128, 128), True),
              ("halo 4x512^2 64->64 3x3", (4, 512, 512, 64, 64), False),
              ("LNet 16x12^2 1024->256 3x3", (16, 12, 12, 1024, 256), False)]
    for name, shp, mod in shapes:
        fns, syms, flops = conv_case(ctx, *shp, modulated=mod)
        r = pairs(name, fns, a.reps, a.pairs, {"kernels": syms, "gflop": round(flops / 1e9, 2)})
        for m in MODES:
            r[f"{m}_tflops"] = round(flops / r[f"{m}_ms"] / 1e9, 1)
        print(json.dumps({"what": name, "tflops": {m: r[f"{m}_tflops"] for m in MODES}}), flush=True)
        torch.cuda.empty_cache()


def flop_share(fn):
    """Share of the conv FLOPs of fn() (run under "f16") per plan precision: {3: single-pass, 2: f16x3 fallback,
    0: exact fp32}."""
    from s2v_amd import ops
    tot = {}

    def hook(c, p, flops, launch):
        tot[p.plan[6]] = tot.get(p.plan[6], 0.0) + flops
        launch()
    with ops.precision("f16"):
        ops.CONV_HOOK = hook
        try:
            fn()
        finally:
            ops.CONV_HOOK = None
    s = sum(tot.values()) or 1.0
    return {str(k): round(v / s, 4) for k, v in sorted(tot.items())}


def time_forwards(a):
    import f16_cases as C
    from s2v_amd import synth

    def dev(x):
        return torch.from_numpy(x).cuda()
    lnet, enet, dnet = C.build_model("lnet"), C.build_model("enet"), C.build_model("dnet")
    mel, face, gt = (dev(x) for x in synth.lipsync_inputs("f16.micro", 16, 256))
    lmel, lface, _ = (dev(x) for x in synth.lipsync_inputs("f16.micro.lnet", 16, 96))
    src, coeff = (dev(x) for x in synth.dnet_inputs("f16.micro", 16, 256))
    cases = [("ENet(+LNet) B=16 256^2", lambda: enet(mel, face, gt)),
             ("LNet B=16 96^2", lambda: lnet(lmel, lface)),
             ("DNet B=16 256^2", lambda: dnet(src, coeff))]
    if not a.no_enhancers:
        from helpers import synth_sd
        from s2v_amd import models
        gfpgan = C.build_model("gfpgan")
        gpen = models.FullGenerator(512, 512, 8, 2)
        gpen.load_state_dict(synth_sd("gpen"), strict=True)
        gpen.eval()
        x4 = dev(synth.face_inputs("f16.micro", 4))

        def enhance():
            gfpgan(x4, return_rgb=False, randomize_noise=False)
            gpen(x4)
        cases.append(("GFPGAN + GPEN B=4 512^2", enhance))
    for name, fn in cases:
        with torch.no_grad():
            share = flop_share(fn)
            pairs(name, {m: fn for m in MODES}, 1, a.pairs, {"conv_flop_share_by_prec": share})
        torch.cuda.empty_cache()


def measure_precision(path):
    import f16_cases as C
    from s2v_amd import ops
    doc = json.load(open(path)) if os.path.exists(path) else {}
    out = {}
    for model in ("lnet", "enet", "dnet", "gfpgan"):
        g = np.load(os.path.join(ROOT, "tests", "golden", C.GOLDEN_OF[model] + ".npz"))
        net = C.build_model(model)
        for mode in ("f16", "f16x3"):
            with ops.precision(mode), torch.no_grad():
                for key, t in C.device_outputs(model, net).items():
                    m, mean = C.golden_error(key, t, g)
                    out.setdefault(mode, {})[key] = {"max": float(f"{m:.3e}"), "mean": float(f"{mean:.3e}")}
                    print(f"{mode} {key}: max {m:.3e} mean {mean:.3e}", flush=True)
    doc["box"] = box()
    doc["device"] = out["f16"]
    doc["device_f16x3"] = out["f16x3"]
    doc["reference"] = "tests/golden (the reference modules' outputs on the synthetic weights and inputs)"
    json.dump(doc, open(path, "w"), indent=1, sort_keys=True)


def emulate(path):
    import f16_cases as C
    doc = json.load(open(path)) if os.path.exists(path) else {}
    emu = {}
    for bits, name in ((11, "emulation"), (8, "emulation_bf16_single_pass")):
        emu[name] = {}
        for model in ("lnet", "enet", "dnet", "gfpgan"):
            for key, (m, mean) in C.emulation_figures(model, bits).items():
                emu[name][key] = {"max": float(f"{m:.3e}"), "mean": float(f"{mean:.3e}")}
                print(f"{bits} bits {key}: max {m:.3e} mean {mean:.3e}", flush=True)
    doc.update(emu)
    doc["emulation_method"] = ("CPU oracle with both operands of every F.conv2d / F.conv_transpose2d rounded to 11 (8) "
                               "significant bits after a power-of-two scale (weights max into [2^13, 2^14), activations "
                               "[2^9, 2^10)), against the plain oracle")
    json.dump(doc, open(path, "w"), indent=1, sort_keys=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--time", action="store_true")
    ap.add_argument("--precision", metavar="JSON")
    ap.add_argument("--emulate", metavar="JSON")
    ap.add_argument("--pairs", type=int, default=20)
    ap.add_argument("--reps", type=int, default=10, help="conv launches per timed graph replay")
    ap.add_argument("--only", choices=["convs", "forwards"], default=None)
    ap.add_argument("--no_enhancers", action="store_true")
    a = ap.parse_args()
    if a.emulate:
        emulate(a.emulate)
    if a.precision:
        measure_precision(a.precision)
    if a.time:
        print(json.dumps({"box": box(), "modes": MODES, "pairs": a.pairs}), flush=True)
        if a.only != "forwards":
            time_convs(a)
        if a.only != "convs":
            time_forwards(a)


if __name__ == "__main__":
    main()
