#!/usr/bin/env python3
"""The geometry between the preprocessing networks, host route against device route (--geometry), in one
session, interleaved, on synthetic weights:

  * landmarks: 16 faces per batch through crop + FAN + peaks + the map back to the frame
    (FaceAlignment.get_landmarks_from_batch, boxes given), host points against on_device=True;
  * 3dmm: 32 frames of 700 x 700 through the 3DMM front end and the ResNet-50: inference._usable_landmarks +
    Face3DExtractor.face_3dmm_extraction against semantic_device; and the front end alone (the per-frame fits
    against one s2v_face3d_align launch);
  * windows: the DNet coefficient windows of a 1 000-frame clip: pipeline.dnet_coefficients + the upload
    against dnet_coefficients_device.

    python tools/geometry_micro.py [--iters 10] [--rounds 2] [--out profiles/geometry_micro.txt]

Every time is a host clock around the call, ended by a device synchronise (the host routes are host work, which
device events do not see); warm, median and minimum of --iters calls, host and device alternating --rounds
times.  One JSON line per measurement, printed and written to --out.
"""
import argparse
import json
import os
import sys
import time
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import s2v_import  # noqa: E402,F401


def clock_ms(fn, iters):
    ts = []
    for _ in range(iters):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    ts.sort()
    return {"median": round(ts[len(ts) // 2], 3), "min": round(ts[0], 3)}


def face_landmarks(rng, n, W, H):
    """Plausible 68-point sets: noise around a face whose seven fitted points sit where a face has them."""
    pts = {30: (0.0, 0.05), 36: (-0.7, -0.45), 39: (-0.3, -0.45), 42: (0.3, -0.45), 45: (0.7, -0.45),
           48: (-0.42, 0.62), 54: (0.42, 0.62)}
    out = np.empty((n, 68, 2), np.float32)
    for i in range(n):
        d, cx, cy = rng.uniform(0.12, 0.3) * W, rng.uniform(0.4, 0.6) * W, rng.uniform(0.4, 0.6) * H
        a = np.deg2rad(rng.uniform(-15, 15))
        out[i] = rng.uniform(-0.6, 0.6, (68, 2)) * d + (cx, cy)
        for k, (u, v) in pts.items():
            out[i, k] = (cx + np.cos(a) * u * d - np.sin(a) * v * d, cy + np.sin(a) * u * d + np.cos(a) * v * d)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "geometry_micro.txt"))
    a = ap.parse_args()
    from s2v_amd import face3d, face_detection as fd, inference, models, ops, pipeline, synth
    from s2v_amd.models.face3d_arch import ReconNetWrapperParams
    from s2v_amd.models.fan_arch import FANParams
    dev = torch.device("cuda")
    lines = []

    def emit(**kw):
        kw = dict(device=torch.cuda.get_device_name(0), precision=ops.PRECISION, iters=a.iters, **kw)
        lines.append(json.dumps(kw))
        print(lines[-1], flush=True)

    # ---- landmarks: 16 faces, fan_micro.py's shape
    B = 16
    net = models.FAN()
    net.load_state_dict(synth.synth_torch_state_dict(FANParams(), **synth.FAN_SYNTH), strict=True)
    fa = fd.FaceAlignment(fd.LandmarksType._2D, device=dev, detector=types.SimpleNamespace(reference_scale=195),
                          fan=net.eval())
    frames = torch.from_numpy(synth.sr_frame("fan.micro", B, 360, 480)).to(dev)
    boxes = [[np.array([150.0 + 3 * i, 90.0 + 2 * i, 330.0 + 3 * i, 290.0 + 2 * i, 0.99], np.float32)] for i in range(B)]
    routes = {"host": lambda: fa.get_landmarks_from_batch(frames, detected_faces=boxes),
              "device": lambda: fa.get_landmarks_from_batch(frames, detected_faces=boxes, on_device=True)}
    same = np.array_equal(np.stack([r[0] for r in routes["host"]()]), routes["device"]()[0].cpu().numpy())
    for fn in routes.values():
        fn()
    for r in range(a.rounds):
        for name, fn in routes.items():
            ms = clock_ms(fn, a.iters)
            emit(stage="landmarks", what="crop + FAN + peaks + back-map, boxes given", geometry=name, faces=B,
                 round=r, ms=ms, faces_per_s=round(B / ms["median"] * 1e3, 1), equal_points=bool(same))

    # ---- 3DMM front end: 32 frames of 700 x 700
    N, W, H = 32, 700, 700
    recon = models.ReconNetWrapper()
    recon.load_state_dict(synth.synth_torch_state_dict(ReconNetWrapperParams(), **synth.RETINA_SYNTH))
    lm3d = inference.LM3D_STANDIN
    ext = face3d.Face3DExtractor(recon.eval(), lm3d, dev)
    rgb = torch.from_numpy(synth.sr_frame("geometry.micro", N, H, W)).to(dev)
    lms = face_landmarks(np.random.default_rng(3), N, W, H)
    lms_dev = torch.from_numpy(lms).to(dev)

    def host_3dmm():
        usable, _ = inference._usable_landmarks(lms, H, W, lm3d)
        return ext.face_3dmm_extraction(rgb, usable)

    def host_fits():
        usable, _ = inference._usable_landmarks(lms, H, W, lm3d)
        return [face3d.align_params(W, H, face3d.frame_landmarks(l, W, H, lm3d), lm3d)[1] for l in usable]

    routes = {"host": host_3dmm, "device": lambda: ext.semantic_device(rgb, lms_dev)}
    fits = {"host": host_fits, "device": lambda: face3d.align_device(ext.ctx, lms_dev, W, H, lm3d)}
    sem_h, (sem_d, status) = routes["host"](), routes["device"]()
    boxes_equal = np.array_equal(np.asarray(fits["host"](), np.int32), fits["device"]()[0].cpu().numpy())
    sem_equal = np.array_equal(sem_h[:, :257], sem_d.cpu().numpy()[:, :257])
    for r in range(a.rounds):
        for name in ("host", "device"):
            ms = clock_ms(routes[name], a.iters)
            emit(stage="3dmm", what="fits + resize-crop + ResNet-50 (host: + copy back)", geometry=name, frames=N,
                 hw=[H, W], round=r, ms=ms, frames_per_s=round(N / ms["median"] * 1e3, 1),
                 equal_boxes=bool(boxes_equal), equal_coefficients=bool(sem_equal),
                 status=np.bincount(status.cpu().numpy(), minlength=3).tolist())
            ms = clock_ms(fits[name], a.iters)
            emit(stage="3dmm front end", what="validation + fits of every frame", geometry=name, frames=N, round=r,
                 ms=ms)

    # ---- DNet coefficient windows of a 1 000-frame clip
    N = 1000
    sem = synth.hash_array("geometry.micro.semantic", (N, 262), -1.0, 1.0).astype(np.float32)
    exp = synth.hash_array("inference.expression", (64,), -1.0, 1.0)
    sem_dev = torch.from_numpy(sem).to(dev)
    routes = {"host": lambda: torch.from_numpy(pipeline.dnet_coefficients(sem, exp, False, 0, N)).to(dev),
              "device": lambda: pipeline.dnet_coefficients_device(sem_dev, exp, False, 0, N)}
    same = torch.equal(routes["host"](), routes["device"]())
    for r in range(a.rounds):
        for name, fn in routes.items():
            ms = clock_ms(fn, max(3, a.iters // 3) if name == "host" else a.iters)
            emit(stage="windows", what="[1000, 73, 26] coefficient windows (host: + upload)", geometry=name, frames=N,
                 round=r, ms=ms, equal_windows=bool(same))

    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("# python tools/geometry_micro.py: host and device geometry routes in one session, alternating;\n"
                "# host clock around each call, ended by a device synchronise; warm; median / min in ms\n")
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
