"""bench.py's multi-process paths on the CPU (gloo, world size 2): the self-spawning launcher
(``bench.py --gpus N`` outside torchrun) and the torchrun launch the driver uses.  Both must print
exactly one JSON line, from rank 0, with n_gpus = the world size the process group saw."""
import json
import os
import socket
import subprocess
import sys

import pytest

from conftest import REPO


def _port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _json_lines(out):
    return [json.loads(line) for line in out.splitlines() if line.startswith("{")]


def _check(r, world):
    assert r.returncode == 0, r.stderr[-3000:]
    lines = _json_lines(r.stdout)
    assert len(lines) == 1, r.stdout
    res = lines[0]
    assert res["n_gpus"] == world and res["config"]["world_size_seen"] == world
    assert res["steps"] == 3 and res["value"] > 0 and res["scaling"] == "weak"
    assert res["config"]["global_batch"] == world * res["config"]["batch_per_gpu"]


ARGS = ["--device", "cpu", "--workload", "selftest", "--steps", "3", "--warmup", "1"]


@pytest.mark.parametrize("world", [1, 2])
def test_self_spawning_launcher(world):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    r = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", str(world)] + ARGS,
                       capture_output=True, text=True, timeout=300, env=env, cwd=REPO)
    _check(r, world)


def test_torchrun_launch():
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
                        "--master-addr", "127.0.0.1", "--master-port", str(_port()),
                        os.path.join(REPO, "bench.py"), "--gpus", "2"] + ARGS,
                       capture_output=True, text=True, timeout=300, env=env, cwd=REPO)
    _check(r, 2)


def test_dump_outputs_and_full(tmp_path):
    """``--dump-outputs DIR`` writes what the last timed step returned as float32 .npy (the self-test's
    step returns sum(arange(64)) = 2016); ``--full`` is accepted, and the line keeps ``ms_per_step``."""
    import numpy as np
    d = tmp_path / "outs"
    r = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--full",
                        "--dump-outputs", str(d)] + ARGS, capture_output=True, text=True, timeout=300, cwd=REPO)
    _check(r, 1)
    res = _json_lines(r.stdout)[0]
    assert res["ms_per_step"] >= 0 and res["steps"] == 3
    files = sorted(os.listdir(d))
    assert files == ["out0.npy"], files
    a = np.load(d / "out0.npy")
    assert a.dtype == np.float32 and a.shape == () and a == 2016.0


def test_dump_outputs_names_dtypes_and_cap(tmp_path):
    """bench.dump_outputs on the forms the workloads' steps return: a tuple named by the workload's
    ``output_names`` (lipsync), the engine's dict named by key (dnet), uint8 -> float32 (pipeline),
    float64 kept, the ``_rank<r>`` suffix, and a tensor above its share of the 64 MB written as the same
    seeded sample of itself on every call, the files staying under the cap."""
    import numpy as np
    import torch

    import bench
    u8 = torch.arange(24, dtype=torch.uint8).reshape(2, 3, 4)
    f64 = torch.linspace(0, 1, 5, dtype=torch.float64)
    d = tmp_path / "tuple"
    bench.dump_outputs((u8, f64), ("out", "low"), str(d), 0, 1)
    assert sorted(os.listdir(d)) == ["low.npy", "out.npy"]
    a, b = np.load(d / "out.npy"), np.load(d / "low.npy")
    assert a.dtype == np.float32 and a.shape == (2, 3, 4) and np.array_equal(a, u8.numpy().astype(np.float32))
    assert b.dtype == np.float64 and np.array_equal(b, f64.numpy())

    d = tmp_path / "dict"                  # names that do not fit the tensor count are not used
    bench.dump_outputs({"fake_image": u8.float(), "flows": [f64, f64 + 1], "note": "x"}, ("out", "low"), str(d), 1, 2)
    assert sorted(os.listdir(d)) == ["fake_image_rank1.npy", "flows0_rank1.npy", "flows1_rank1.npy"]
    assert np.array_equal(np.load(d / "flows1_rank1.npy"), f64.numpy() + 1)

    d = tmp_path / "pos"
    bench.dump_outputs([u8, (u8 + 1,)], (), str(d), 0, 1)
    assert sorted(os.listdir(d)) == ["out0.npy", "out1.npy"]
    assert np.array_equal(np.load(d / "out1.npy"), (u8 + 1).numpy().astype(np.float32))

    big = torch.arange(20_000_000, dtype=torch.int32).reshape(1000, -1)      # 80 MB as float32
    d1, d2 = tmp_path / "big1", tmp_path / "big2"
    bench.dump_outputs((big, u8), ("big", "small"), str(d1), 0, 1)
    bench.dump_outputs((big, u8), ("big", "small"), str(d2), 0, 1)
    s1, s2 = np.load(d1 / "big.npy"), np.load(d2 / "big.npy")
    assert sum(os.path.getsize(d1 / f) for f in os.listdir(d1)) <= bench.DUMP_BYTES
    assert s1.dtype == np.float32 and s1.ndim == 1 and 7_000_000 < s1.size < big.numel()
    assert np.array_equal(s1, s2)
    idx = s1.astype(np.int64)              # the values are their own flat indices (exact in float32 below 2^24)
    assert np.all(np.diff(idx) >= 0) and idx.min() < 100_000 and idx.max() > 19_900_000
    assert np.array_equal(np.load(d1 / "small.npy"), u8.numpy().astype(np.float32))

    # rank 0 with nothing to write is an error; another rank of the clip workload holds no frames
    with pytest.raises(RuntimeError):
        bench.dump_outputs(None, (), str(tmp_path / "none"), 0, 2)
    with pytest.raises(RuntimeError):
        bench.dump_outputs({"note": "x"}, (), str(tmp_path / "none"), 0, 1)
    bench.dump_outputs(None, (), str(tmp_path / "none"), 1, 2)
    assert not os.path.exists(tmp_path / "none")


@pytest.mark.gpu
@pytest.mark.parametrize("full", [False, True])
def test_plain_and_full_result_lines(full, tmp_path, monkeypatch, capsys):
    """A plain run's line has the headline fields only; ``--full`` adds ``roofline``, ``alt_precision``
    and ``cpu_baseline``.  Both write the step's outputs (DNet's dict, named by key).  In-process on
    the smallest workload (dnet, B = 2)."""
    import numpy as np

    import bench
    argv = ["bench.py", "--workload", "dnet", "--batch", "2", "--steps", "2", "--warmup", "1", "--cpu-seconds", "0.1",
            "--dump-outputs", str(tmp_path)] + (["--full"] if full else [])
    monkeypatch.setattr(sys, "argv", argv)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    bench.main()
    res = _json_lines(capsys.readouterr().out)
    assert len(res) == 1
    res = res[0]
    assert res["steps"] == 2 and res["ms_per_step"] > 0 and res["dtype"] == "f32" and res["higher_is_better"] is True
    assert abs(res["value"] * res["ms_per_step"] / (1e3 * 2) - 1) < 0.01      # value = frames / elapsed
    for k in ("roofline", "alt_precision", "cpu_baseline"):
        assert (k in res) == full, (k, sorted(res))
    a = np.load(tmp_path / "fake_image.npy")
    assert a.dtype == np.float32 and a.shape == (2, 3, 256, 256) and np.isfinite(a).all() and a.std() > 0


def test_dump_stamps_needs_full():
    r = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--dump-stamps", "x.json"] + ARGS,
                       capture_output=True, text=True, timeout=120, cwd=REPO)
    assert r.returncode != 0 and "--full" in (r.stderr + r.stdout)


def test_cpu_device_is_selftest_only():
    r = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--device", "cpu", "--workload", "lipsync"],
                       capture_output=True, text=True, timeout=120, cwd=REPO)
    assert r.returncode != 0 and "selftest" in (r.stderr + r.stdout)
