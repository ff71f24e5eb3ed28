"""Host side of the FAN landmark path: the parameter manifest and strict loading, the crop-window and
heatmap-to-frame arithmetic against tests/golden/fan_goldens.npz (recorded from the reference's
utils.transform / crop / get_preds_fromhm by tests/golden/make_fan_golden.py), KeypointExtractor's rules,
the C ABI's argument validation, the CLI flags and a dry run of the engine's host plan."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import fan_cases as FC
import s2v_import  # noqa: F401

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


# ----------------------------------------------------------------------------- parameters
def test_state_dict_manifest_is_strict():
    from s2v_amd import models
    from s2v_amd.models.fan_arch import FANParams, conv_blocks
    with open(os.path.join(GOLDEN, "fan_keys.json")) as f:
        want = json.load(f)
    mine = {k: list(v.shape) for k, v in FANParams(4).state_dict().items()}
    assert mine == want and len(want) == 1129
    for k in ("conv1.weight", "bn1.running_var", "conv2.bn1.weight", "conv2.downsample.2.weight", "m0.b1_4.conv1.weight",
              "m3.b2_plus_1.bn3.bias", "top_m_0.conv3.weight", "conv_last0.bias", "bn_end0.weight", "l0.weight",
              "bl0.weight", "al2.bias", "l3.bias"):
        assert k in want, k
    assert "bl3.weight" not in want and "al3.weight" not in want        # the last stack feeds nothing
    assert conv_blocks(4) == 59
    net = models.FAN()
    net.load_state_dict(dict(FC.state_dict()), strict=True)
    sd = dict(FC.state_dict())
    del sd["m2.b3_2.bn2.running_mean"]
    with pytest.raises(RuntimeError, match="m2.b3_2.bn2.running_mean"):
        models.FAN().load_state_dict(sd, strict=True)
    with pytest.raises(RuntimeError, match="extra"):
        models.FAN().load_state_dict(dict(FC.state_dict(), extra=torch.zeros(1)), strict=True)


def test_load_fan_takes_both_file_forms_and_is_strict(tmp_path):
    from s2v_amd import models
    sd = FC.state_dict()
    torch.save(sd, tmp_path / "plain.pth")
    torch.save({"state_dict": sd}, tmp_path / "wrapped.pth")
    for name in ("plain.pth", "wrapped.pth"):
        net = models.load_fan(str(tmp_path / name))
        assert not net.training and torch.equal(net.l3.bias, sd["l3.bias"])
    torch.save({k: v for k, v in sd.items() if k != "al1.weight"}, tmp_path / "bad.pth")
    with pytest.raises(RuntimeError, match="al1.weight"):
        models.load_fan(str(tmp_path / "bad.pth"))


def test_input_sides_must_be_multiples_of_64():
    from s2v_amd.models import fan_arch
    for hw in ((256, 256), (128, 128), (64, 192)):
        fan_arch.check_input(*hw)
    for hw in ((255, 256), (256, 96), (0, 64)):
        with pytest.raises(ValueError, match="multiples of 64"):
            fan_arch.check_input(*hw)


# ----------------------------------------------------------------------------- host arithmetic
def test_crop_table_matches_reference_windows(golden):
    from s2v_amd import face_detection as fd
    g = golden("fan_goldens")
    cs = [fd.box_center_scale(b[1:]) for b in FC.CROP_BOXES]
    table = fd.crop_table([b[0] for b in FC.CROP_BOXES], [c for c, _ in cs], [s for _, s in cs], FC.CROP[2:])
    assert table.dtype == np.int32 and np.array_equal(table, g["crop_table"])
    # the cases are what they claim: inside, over each edge, larger than the frame
    H, W = FC.CROP[2:]
    t = table[:, 1:]
    inside = lambda r: (r[0] >= 0, r[1] >= 0, r[2] <= W, r[3] <= H)  # noqa: E731
    assert inside(t[0]) == (True, True, True, True)
    assert inside(t[1]) == (False, True, True, True) and inside(t[2]) == (True, False, True, True)
    assert inside(t[3]) == (True, True, False, True) and inside(t[4]) == (True, True, True, False)
    assert t[5, 0] < 0 and t[5, 1] < 0 and t[5, 2] > W and t[5, 3] > H


def test_box_center_scale_states_the_glue_facts():
    from s2v_amd import face_detection as fd
    assert fd.CENTER_Y_SHIFT == 0.12 and fd.HEATMAP_STACK == -1 and fd.FAN_RESOLUTION == 256.0
    c, s = fd.box_center_scale([10.0, 20.0, 110.0, 220.0, 0.9])
    assert c.dtype == torch.float32 and c.tolist() == [60.0, 120.0 - 0.12 * 200.0]
    assert s == (100.0 + 200.0) / 195
    assert sorted(fd.FLIP_PAIRS) == list(range(68)) and fd.FLIP_PAIRS[0] == 16 and fd.FLIP_PAIRS[36] == 45
    assert all(fd.FLIP_PAIRS[fd.FLIP_PAIRS[k]] == k for k in range(68))


def test_empty_or_missing_window_raises_before_any_launch():
    from s2v_amd import face_detection as fd
    c = torch.tensor([40.5, 40.5])                    # a 0.2-pixel window between two integers
    with pytest.raises(ValueError, match="empty window"):
        fd.crop_table([0], [c], [0.001], (90, 120))
    with pytest.raises(ValueError, match="misses"):
        fd.crop_table([0], [torch.tensor([-400.0, 40.0])], [0.5], (90, 120))


def test_preds_map_back_to_frame_coordinates(golden):
    from s2v_amd import face_detection as fd
    g = golden("fan_goldens")
    got = fd.preds_to_image(torch.from_numpy(g["full_preds"]), torch.tensor(FC.FULL_CENTER), FC.FULL_SCALE, 64)
    assert got.dtype == torch.float32 and np.array_equal(got.numpy(), g["full_preds_orig"])
    assert np.array_equal(g["full_preds_orig"], np.trunc(g["full_preds_orig"]))


# ----------------------------------------------------------------------------- KeypointExtractor
class _FakeDetector:
    def __init__(self, per_frame):
        self.per_frame = list(per_frame)
        self.seen = 0

    def get_landmarks_from_batch(self, images):
        out = self.per_frame[self.seen: self.seen + len(images)]
        self.seen += len(images)
        return out


def test_keypoint_extractor_minus_one_and_reuse_rules(tmp_path):
    from s2v_amd.face3d import KeypointExtractor
    a = np.arange(136, dtype=np.float32).reshape(68, 2)
    b = a + 1000
    frames = [np.zeros((8, 8, 3), np.uint8)] * 6
    det = _FakeDetector([None, [a, b], None, None, [b], None])
    kp = KeypointExtractor(det, batch=4)
    out = kp.extract_keypoint(frames, name=str(tmp_path / "clip.mp4"), info=False)
    assert out.shape == (6, 68, 2) and kp.misses == 4
    assert (out[0] == -1).all()                       # no face and nothing earlier: all -1
    assert np.array_equal(out[1], a)                  # the first face of the frame
    assert np.array_equal(out[2], a) and np.array_equal(out[3], a)      # no face: the previous frame's points
    assert np.array_equal(out[4], b) and np.array_equal(out[5], b)
    assert np.array_equal(np.loadtxt(tmp_path / "clip.txt"), out.reshape(-1))
    one = KeypointExtractor(_FakeDetector([None])).extract_keypoint(frames[0])
    assert one.shape == (68, 2) and (one == -1).all()
    arr = KeypointExtractor(_FakeDetector([[a], None])).extract_keypoint(np.zeros((2, 8, 8, 3), np.uint8))
    assert np.array_equal(arr[0], a) and np.array_equal(arr[1], a)


def test_face_alignment_without_fan_raises():
    from s2v_amd import face_detection as fd, models
    fa = fd.FaceAlignment(fd.LandmarksType._2D, device="cpu", detector=fd.SFDDetector("cpu", net=models.S3FD()))
    with pytest.raises(RuntimeError, match="no FAN network"):
        fa.get_landmarks_from_image(np.zeros((64, 64, 3), np.uint8))
    with pytest.raises(FileNotFoundError):
        fd.FaceAlignment(fd.LandmarksType._2D, device="cpu", detector=fa.face_detector, path_to_fan="/nonexistent/2DFAN4.pth")


def test_unusable_landmark_fits_become_the_no_landmark_marker():
    """A face-like landmark set is kept; points no face could give (all in one spot: a degenerate POS fit, or
    a face 20x larger than the frame: a downscale past the resize kernel's limit) become all -1 and are counted."""
    from s2v_amd import inference
    lm3d = inference.LM3D_STANDIN
    H, W = 180, 200
    face = np.zeros((68, 2), np.float32)
    idx = np.array([31, 37, 40, 43, 46, 49, 55]) - 1
    # nose, both corners of each eye, the mouth corners at the stand-in's x / y (y up), 90 px per unit
    pts = {30: lm3d[2], 36: lm3d[0], 39: lm3d[0], 42: lm3d[1], 45: lm3d[1], 48: lm3d[3], 54: lm3d[4]}
    assert sorted(pts) == sorted(idx.tolist())
    for k, p in pts.items():
        face[k] = (100 + 90 * p[0], 90 - 90 * p[1])
    spot = np.full((68, 2), 50.0, np.float32)
    huge = (face - (100, 90)) * 20 + (100, 90)
    none = np.full((68, 2), -1.0, np.float32)
    out, rejects = inference._usable_landmarks(np.stack([face, spot, none, huge.astype(np.float32)]), H, W, lm3d)
    assert rejects == 2 and np.array_equal(out[0], face) and (out[1] == -1).all() and (out[3] == -1).all()
    assert (out[2] == -1).all()


# ----------------------------------------------------------------------------- C ABI
def test_fan_entry_points_reject_bad_arguments():
    from s2v_amd import _lib
    lib = _lib.load()
    p = lambda a: a.ctypes.data  # noqa: E731
    x = np.zeros(4096, np.float32)
    y = np.zeros(4096, np.float32)
    s = np.zeros(64, np.float32)
    t = np.zeros(64, np.float32)
    assert all(a.ctypes.data % 16 == 0 for a in (x, y, s, t))
    bn = lambda *a: lib.s2v_bn_act_nhwc(*a, None)  # noqa: E731
    assert bn(None, 4, 16, 32, 0, p(s), p(t), p(y), 32, 0) == -1
    assert bn(p(x), 4, 16, 32, 0, None, p(t), p(y), 32, 0) == -1
    assert bn(p(x), 4, 16, 32, 0, p(s), p(t), None, 32, 0) == -1
    assert bn(p(x), 0, 16, 32, 0, p(s), p(t), p(y), 32, 0) == -1
    assert bn(p(x), 4, 18, 32, 0, p(s), p(t), p(y), 32, 0) == -1
    assert b"multiple of 4" in lib.s2v_last_error()
    assert bn(p(x), 4, 16, 32, 20, p(s), p(t), p(y), 32, 0) == -1          # the view leaves its pitch
    assert bn(p(x), 4, 16, 32, 0, p(s), p(t), p(y), 32, 18) == -1          # offset not a multiple of 4
    assert bn(p(x), 4, 16, 30, 0, p(s), p(t), p(y), 32, 0) == -1           # pitch not a multiple of 4
    assert bn(p(x) + 4, 4, 16, 32, 0, p(s), p(t), p(y), 32, 0) == -1       # misaligned
    assert b"aligned" in lib.s2v_last_error()

    def mg(a=p(x), b=None, half=0, n=1, h=4, w=4, c=16, s_=p(y), sa=None, sA=None, tA=None, p_=None, pa=None, sB=None,
           tB=None, cs=16):
        return lib.s2v_fan_merge(a, cs, b, cs, half, n, h, w, c, s_, cs, sa, cs, sA, tA, p_, cs, pa, cs, sB, tB, None)
    assert mg(a=None) == -1
    assert mg(s_=None) == -1 and b"no output" in lib.s2v_last_error()
    assert mg(half=1) == -1                                                # b_half without b
    assert mg(c=18, cs=20) == -1
    assert mg(cs=12) == -1                                                 # pitch below the channels
    assert mg(sa=p(y)) == -1                                               # activated output without scale / shift
    assert mg(pa=p(y), sB=p(s)) == -1
    assert mg(h=3, p_=p(y)) == -1 and b"even" in lib.s2v_last_error()      # pooling an odd map
    assert mg(b=p(x), half=1, w=5) == -1
    assert mg(a=p(x) + 4) == -1

    u8 = np.zeros(2 * 8 * 8 * 3, np.uint8)
    out = np.zeros(256 * 256 * 4, np.float32)

    def crop(rows, frames=p(u8), n=2, table=True, y_=p(out)):
        tab = np.asarray(rows, np.int32).reshape(-1, 5)
        return lib.s2v_fan_crop(frames, n, 8, 8, p(tab) if table else None, p(tab), len(tab), y_, None)
    assert crop([(0, 0, 0, 8, 8)], frames=None) == -1
    assert crop([(0, 0, 0, 8, 8)], table=False) == -1
    assert crop([(0, 0, 0, 8, 8)], y_=None) == -1
    assert crop([(2, 0, 0, 8, 8)]) == -1 and b"frame 2" in lib.s2v_last_error()
    assert crop([(0, 0, 0, 8, 8), (1, 5, 0, 5, 8)]) == -1 and b"face 1" in lib.s2v_last_error()   # empty window
    assert crop([(0, 0, 6, 8, 2)]) == -1
    assert crop([(0, 0, 0, 1 << 25, 8)]) == -1

    pr = np.zeros(68 * 2, np.float32)
    va = np.zeros(68, np.float32)
    assert lib.s2v_fan_peaks(None, 1, 64, 64, 68, 68, p(pr), p(va), None) == -1
    assert lib.s2v_fan_peaks(p(x), 1, 64, 64, 68, 68, None, p(va), None) == -1
    assert lib.s2v_fan_peaks(p(x), 1, 64, 64, 68, 68, p(pr), None, None) == -1
    assert lib.s2v_fan_peaks(p(x), 0, 64, 64, 68, 68, p(pr), p(va), None) == -1
    assert lib.s2v_fan_peaks(p(x), 1, 32, 32, 68, 68, p(pr), p(va), None) == -1
    assert b"64x64" in lib.s2v_last_error()
    assert lib.s2v_fan_peaks(p(x), 1, 64, 64, 68, 64, p(pr), p(va), None) == -1          # pitch below the channels


# ----------------------------------------------------------------------------- CLI
def test_cli_parser_accepts_the_landmarks_flag():
    import inspect
    from s2v_amd import inference
    ap = inference.build_parser()
    assert ap.parse_args(["--face", "v.mp4", "--audio", "a.wav"]).landmarks is False
    assert ap.parse_args(["--face", "v.mp4", "--audio", "a.wav", "--landmarks"]).landmarks is True
    sig = inspect.signature(inference.run).parameters
    assert sig["landmarks"].default is False and sig["landmark_detector"].default is None
    assert inspect.signature(inference._semantic).parameters["lms"].default is None


def test_run_without_landmarks_never_imports_the_fan_engine():
    """run() with the option off must not touch the FAN engine: a stub run in a fresh interpreter (the
    device stages replaced by no-ops up to _semantic) leaves s2v_amd.engine.fan unimported."""
    code = """
import sys
import s2v_import
import numpy as np
from s2v_amd import inference
class Stop(Exception): pass
seen = {}
def semantic(frames, ckpt_dir, dev, lms=None):
    seen['lms'] = lms
    raise Stop
inference._semantic = semantic
inference._frames = lambda face, n: (np.zeros((2, 64, 64, 3), np.uint8), 25.0, 'stub')
inference.load_wav = lambda path, sr: np.zeros(16000, np.float32)
import torch
from s2v_amd import audio, post
audio.melspectrogram = lambda wav: torch.zeros(80, 80)
audio.mel_chunks = lambda mel, fps: torch.zeros(4, 80, 16)
post.resize_linear = lambda *a, **k: None
class _Lib:
    def s2v_u8_to_gan(self, *a): return 0
class _Ctx:
    lib = _Lib(); stream = None
post._ctx = lambda dev: _Ctx()
inference._weights = lambda d: (None, None, 'stub')
try:
    inference.run('v.npy', 'a.wav', device='cpu')
except Stop:
    pass
assert seen == {'lms': None}, seen
assert 's2v_amd.engine.fan' not in sys.modules, 'FAN engine imported without --landmarks'
print('ok')
"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-c", code], cwd=root, capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout + r.stderr


# ----------------------------------------------------------------------------- engine host plan
@pytest.mark.parametrize("n,size", [(2, 128), (1, 256), (1, 64)])
def test_fan_engine_plan_runs_dry_within_the_launch_budget(monkeypatch, n, size):
    """The engine's shape / view bookkeeping on CPU with no-op launches (as test_engine_dryrun.py), counting
    launches: at most 7 per ConvBlock (59 of them), 9 per stack outside its blocks and 3 for the stem = 452.
    A 64x64 input reaches 1x1 maps at the hourglass bottom."""
    from test_engine_dryrun import _NoLib, _NoOps
    from s2v_amd import ops
    from s2v_amd.engine import fan
    lib = _NoLib()
    monkeypatch.setattr(ops, "S2V", _NoOps(lib.calls))
    monkeypatch.setattr(ops, "_require_cuda", lambda t, what: None)
    monkeypatch.setattr(ops._lib, "load", lambda: lib)
    monkeypatch.setattr(ops.Ctx, "stream", property(lambda self: ctypes.c_void_p(0)))
    eng = fan.FANEngine(FC.state_dict(), "cpu")
    ctx = ops.Ctx("cpu")
    x4 = ops.NHWC(torch.zeros(n, size, size, 4))
    eng.forward(ctx, x4)            # the first forward also packs the split weights and measures the ranges
    first = dict(lib.calls)
    assert first["split_weights_"] == first["conv2d_"]
    maps = eng.forward(ctx, x4)
    assert [(m.n, m.h, m.w, m.cs) for m in maps] == [(n, size // 4, size // 4, 68)] * 4
    for k in lib.calls:
        lib.calls[k] -= first[k]
    total = sum(lib.calls.values())
    assert fan.LAUNCH_BUDGET == 7 * 59 + 9 * 4 + 3 == 452
    print(f"FAN-4 forward: {total} launches {dict(lib.calls)}")
    assert total <= 452 and lib.calls["split_weights_"] == 0 and lib.calls.get("amax_", 0) == 0
    # 59 blocks x 3 convs + 2 downsample convs + stem + per stack conv_last, l (+ bl, al on the first three)
    # (conv2 and conv4 are the two blocks with a downsample: its BN pass, and the 1x1 conv in place of the merge)
    assert lib.calls["conv2d_"] == 59 * 3 + 2 + 1 + 4 * 2 + 3 * 2
    assert lib.calls["s2v_bn_act_nhwc"] == 59 * 2 + 2 + 1
    assert lib.calls["s2v_fan_merge"] == (59 - 2) + 1 + 4 * (1 + 4)
    assert [tuple(o.shape) for o in eng.to_nchw(maps)] == [(n, 68, size // 4, size // 4)] * 4
    before = dict(lib.calls)
    with pytest.raises(ValueError, match="multiples of 64"):
        eng.forward(ctx, ops.NHWC(torch.zeros(1, 96, 128, 4)))
    assert lib.calls == before
