"""The device NMS without a GPU: the NumPy restatement of s2v_nms's contract (nms_cases.contract) against
face.py_cpu_nms and the reference's recorded keep lists, the nms= / S2V_NMS validation of the three
detectors and of inference.run, and the C ABI's argument checks."""
import ctypes
import os

import numpy as np
import pytest
import torch

import nms_cases as NC
import s2v_import  # noqa: F401
import s3fd_cases as SC


@pytest.mark.parametrize("k", [1, 2, 3, 17, 64, 65, 300, 1000])
@pytest.mark.parametrize("thresh", [0.3, 0.4])
def test_contract_equals_py_cpu_nms_on_distinct_scores(k, thresh):
    for rs in (8, 16):
        rows = NC.clustered(1000 * rs + k, k, rs)
        assert NC.distinct_scores(rows)
        exp = NC.by_py_cpu_nms(rows, thresh)
        got, kept, status = NC.contract(rows, thresh)
        assert status == NC.OK and kept == len(exp)
        assert np.array_equal(got.view(np.uint32), exp.view(np.uint32))
        if k >= 64:
            assert 1 < kept < k                                            # the sweep suppresses and keeps
        # S3FD's pre-filter: dropping score <= 0.5 first equals dropping it after the NMS
        pre, _, _ = NC.contract(rows, thresh, min_score=0.5)
        assert np.array_equal(pre, exp[exp[:, 5] > 0.5])


def test_contract_top_k_and_keep_max_equal_the_retinaface_postprocess():
    from s2v_amd import face
    rows = NC.clustered(77, 400, 16)
    r = NC.position_sorted(rows)
    dets, landms = face.nms_postprocess(r[:, 1:5], r[:, 5], r[:, 6:16], 0.4, top_k=150, keep_top_k=20)
    got, kept, status = NC.contract(rows, 0.4, top_k=150, keep_max=20)
    assert status == NC.OK and kept > 20 and len(got) == 20
    assert np.array_equal(got[:, 1:6], dets)
    assert np.array_equal(got[:, 6:16].reshape(-1, 5, 2).transpose(0, 2, 1).reshape(-1, 10), landms)


@pytest.mark.parametrize("case", sorted(SC.CASES))
def test_contract_equals_the_recorded_keep_lists(golden, case):
    g = golden("s3fd_goldens")
    for i in range(SC.CASES[case][1]):
        cand, idx = g[f"{case}_cand{i}"], g[f"{case}_cand_idx{i}"]
        rows = np.zeros((len(cand), 8), np.float32)
        rows[:, 0] = idx.astype(np.int32).view(np.float32)
        rows[:, 1:6] = cand
        assert (np.diff(idx) > 0).all() and NC.distinct_scores(rows)
        shuffled = rows[np.random.default_rng(i).permutation(len(rows))]
        got, kept, status = NC.contract(shuffled, 0.3)
        assert status == NC.OK and kept == len(got) > 0
        assert NC.position_index(got).tolist() == idx[g[f"{case}_nms_keep{i}"]].tolist()
        pre, _, _ = NC.contract(shuffled, 0.3, min_score=0.5)
        assert np.array_equal(pre[:, 1:6], g[f"{case}_dets{i}"])


def test_contract_tie_order_nan_and_capacity():
    rows = NC.disjoint([0.5, 0.9, 0.5, 0.9, 0.5])                          # position indices 3 5 7 9 11
    got, kept, _ = NC.contract(rows[[4, 0, 3, 1, 2]], 0.3)
    assert kept == 5 and NC.position_index(got).tolist() == [9, 5, 11, 7, 3]
    got, _, _ = NC.contract(NC.disjoint([0.0, -0.0, 0.0]), 0.3)
    assert NC.position_index(got).tolist() == [7, 5, 3]                    # -0 ties with +0
    bad = NC.disjoint([0.5, np.nan])
    assert NC.contract(bad, 0.3)[1:] == (0, NC.NAN_SCORE) and NC.contract(bad, 0.3, min_score=0.7)[2] == NC.NAN_SCORE
    assert NC.contract(NC.disjoint(np.linspace(0.1, 0.9, 9)), 0.3, capacity=8)[2] == NC.OVER_CAPACITY
    assert NC.contract(NC.disjoint(np.linspace(0.1, 0.9, 9)), 0.3, min_score=0.15, capacity=8)[2] == NC.OK
    assert NC.contract(NC.disjoint(np.linspace(0.1, 0.9, 9)), 0.3, top_k=8, capacity=8)[1:] == (8, NC.OK)
    assert NC.contract(NC.disjoint(np.linspace(0.1, 0.9, 9)), 0.3, top_k=9, capacity=8)[2] == NC.OVER_CAPACITY


def test_nms_argument_and_environment_validation(monkeypatch):
    from s2v_amd import face, face_detection, inference, restore
    monkeypatch.delenv("S2V_NMS", raising=False)
    assert face.nms_mode() == "host" and face.nms_mode(None) == "host" and face.nms_mode("device") == "device"
    with pytest.raises(ValueError, match="S2V_NMS"):
        face.nms_mode("gpu")
    monkeypatch.setenv("S2V_NMS", "device")
    assert face.nms_mode(None) == "device" and face.nms_mode("host") == "host"
    monkeypatch.setenv("S2V_NMS", "Device")
    with pytest.raises(ValueError, match="S2V_NMS"):
        face.nms_mode(None)
    net = torch.nn.Identity()
    for build in (lambda nms: face_detection.SFDDetector("cpu", net=net, nms=nms),
                  lambda nms: face.RetinaFaceDetection(device="cpu", net=net, nms=nms),
                  lambda nms: restore.RetinaFaceDetector(device="cpu", net=net, nms=nms)):
        with pytest.raises(ValueError, match="S2V_NMS"):
            build(None)
        with pytest.raises(ValueError, match="S2V_NMS"):
            build("cuda")
        assert build("host").nms == "host" and build("device").nms == "device"
    monkeypatch.setenv("S2V_NMS", "device")
    assert face_detection.SFDDetector("cpu", net=net).nms == "host"       # the default is "host", not the variable
    assert face_detection.SFDDetector("cpu", net=net, nms=None).nms == "device"
    with pytest.raises(ValueError, match="S2V_NMS"):                       # before any file is opened
        inference.run("no_such.mp4", "no_such.wav", nms="fast")
    a = inference.build_parser().parse_args(["--face", "f", "--audio", "a", "--nms", "device"])
    assert a.nms == "device"
    assert inference.build_parser().parse_args(["--face", "f", "--audio", "a"]).nms is None
    with pytest.raises(SystemExit):
        inference.build_parser().parse_args(["--face", "f", "--audio", "a", "--nms", "gpu"])


def test_lib_lists_s2v_nms_and_the_header_declares_it():
    from s2v_amd import _lib
    assert "s2v_nms" in _lib.EXPORTS and "s2v_nms_capacity" in _lib.EXPORTS
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "include", "s2v.h")) as f:
        header = f.read()
    assert "int s2v_nms(const float *cand, const int *count, int n, int max_cand, int row_stride," in header
    assert "int s2v_nms_capacity(void);" in header


def test_s2v_nms_refuses_bad_arguments_before_any_launch():
    from s2v_amd import _lib
    lib = _lib.load()
    assert lib.s2v_nms_capacity() >= 5000                                  # RetinaFace's top_k
    buf = (ctypes.c_float * 64)()
    cnt = (ctypes.c_int * 4)()
    p = ctypes.addressof
    ok = dict(cand=p(buf), count=p(cnt), n=1, max_cand=4, rs=8, thr=0.3, ms=0.5, top_k=0, keep_max=4, out=p(buf),
              kept=p(cnt), status=p(cnt))

    def call(**kw):
        a = dict(ok, **kw)
        return lib.s2v_nms(a["cand"], a["count"], a["n"], a["max_cand"], a["rs"], a["thr"], a["ms"], a["top_k"],
                           a["keep_max"], a["out"], a["kept"], a["status"], None)
    for kw in (dict(cand=None), dict(count=None), dict(out=None), dict(kept=None), dict(status=None), dict(n=0),
               dict(max_cand=0), dict(keep_max=0), dict(top_k=-1), dict(rs=5), dict(rs=65), dict(thr=float("nan")),
               dict(ms=float("nan")), dict(max_cand=(1 << 24) + 1)):
        assert call(**kw) == -1, kw
        assert b"nms" in lib.s2v_last_error()
