"""CPU tests of the opt-in single-pass f16 conv arithmetic ("f16", S2V_PREC_F16 = 3): the mode's name and
code, the environment default, and what the planner answers for it (s2v_conv2d_plan, host only): exactly
the f16x3 plan, with out[6] = 3 where the launch runs single-pass (conv_igemm_x3 tiles, conv_x3_halo)
and 2 where it falls back to f16x3 (conv_x3_nar, conv_head_x3, x_split inputs)."""
import ctypes
import os
import subprocess
import sys

import pytest

import s2v_import  # noqa: F401
from conftest import REPO
from s2v_amd import _lib, ops


def _plan(n, h, w, cin, cout, k=3, stride=1, pad=1, force_tile=0, in_scale=False, batch=0, prec=3, grid_cap=0,
          x_split=0):
    """s2v_conv2d_plan of a direct conv (the helper of tests/test_host.py, with the precision a parameter)."""
    lib = _lib.load()
    p = _lib.ConvParams()
    p.x, p.y, p.wt_x3, p.wt = 1 << 20, 2 << 20, 3 << 20, 4 << 20
    p.n, p.h, p.w, p.cin, p.xcs = n, h, w, cin, cin
    p.kh = p.kw = k
    p.sh = p.sw = stride
    p.ph = p.pw = pad
    p.dh = p.dw = 1
    p.oh, p.ow = (h + 2 * pad - k) // stride + 1, (w + 2 * pad - k) // stride + 1
    p.cout, p.ycs = cout, cout
    p.kpad = (k * k * cin + 31) // 32 * 32
    p.npad = (cout + 127) // 128 * 128 if cout <= 128 else (cout + 255) // 256 * 256
    p.prec = prec
    p.force_tile = force_tile
    p.grid_cap = grid_cap
    p.x_split = x_split
    if batch:
        p.batch, p.x_bs, p.y_bs, p.w_bs = batch, n * h * w * cin, n * p.oh * p.ow * cout, p.npad * p.kpad
    if in_scale:
        p.in_scale, p.in_scale_ns = 5 << 20, cin
    out = (ctypes.c_int * 11)()
    rc = lib.s2v_conv2d_plan(ctypes.byref(p), out)
    return rc, list(out), lib.s2v_conv2d_ws_bytes(ctypes.byref(p))


def test_precision_name_round_trips():
    assert _lib.PREC_F16 == 3 and ops._PRECISIONS["f16"] == 3
    prev = ops.set_precision("f16")
    try:
        assert ops.PRECISION == "f16" and ops.prec_code() == 3
        assert ops.layout_code(ops.prec_code()) == _lib.PREC_F16X3      # weights / pre-scales: those of f16x3
        assert ops.guard_active() == ops.RANGE_GUARD                    # the f16 range guard covers the mode
        assert ops.set_precision(prev) == "f16"
    finally:
        ops.set_precision(prev)
    assert ops.PRECISION == prev
    with ops.precision("f16"):
        assert ops.prec_code() == 3
    assert ops.PRECISION == prev


def test_bad_precision_name_is_rejected():
    prev = ops.PRECISION
    for bad in ("f16x1", "fp16", "tf32", ""):
        with pytest.raises(ValueError, match="f16") as e:
            ops.set_precision(bad)
        for name in ("f16x3", "bf16x3", "f32", "'f16'"):                # the message lists the four names
            assert name in str(e.value), str(e.value)
    assert ops.PRECISION == prev


def test_environment_selects_the_mode():
    env = dict(os.environ, S2V_PRECISION="f16")
    code = "import s2v_import; from s2v_amd import ops; print(ops.PRECISION, ops.prec_code())"
    r = subprocess.run([sys.executable, "-c", code], cwd=REPO, env=env, capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.split() == ["f16", "3"], (r.stdout, r.stderr[-1000:])
    env["S2V_PRECISION"] = "f16x2"
    r = subprocess.run([sys.executable, "-c", code], cwd=REPO, env=env, capture_output=True, text=True)
    assert r.returncode != 0 and "S2V_PRECISION must be one of" in r.stderr and "'f16'" in r.stderr


# the headline shapes: halo (64 and 128 channels), the 400^2 per-sample-weight StyleConv, a 12^2 LNet conv,
# a persistent (grid_cap) 256x256 launch and a forced tile with split-K
SINGLE_PASS = [
    dict(args=(4, 512, 512, 128, 64)),
    dict(args=(4, 256, 256, 128, 128)),
    dict(args=(1, 400, 400, 128, 128), batch=16),
    dict(args=(16, 12, 12, 1024, 256)),
    dict(args=(16, 200, 200, 256, 256), grid_cap=128),
    dict(args=(2, 16, 16, 64, 128), force_tile=2),
]


@pytest.mark.parametrize("case", SINGLE_PASS, ids=[str(i) for i in range(len(SINGLE_PASS))])
def test_plan_equals_f16x3_plan_but_for_the_precision(case):
    kw = {k: v for k, v in case.items() if k != "args"}
    rc3, p3, ws3 = _plan(*case["args"], prec=3, **kw)
    rc2, p2, ws2 = _plan(*case["args"], prec=2, **kw)
    assert rc3 == 0 and rc2 == 0, _lib.load().s2v_last_error()
    assert p2[6] == 2 and p3[6] == 3, (p2, p3)                 # tile / halo routes run single-pass
    assert p3[:6] + p3[7:] == p2[:6] + p2[7:] and ws3 == ws2, (p2, p3)
    assert p3[0] > 0 and p3[3] in (0, 1, 2, 3, 4, 8), p3     # conv_igemm_x3 A modes, or conv_x3_halo
    if case.get("grid_cap"):
        assert p3[10] == 128 and "conv_igemm_x3_persist<256, 256," in ops.plan_symbol(p3)
    assert ops.plan_symbol(p3).endswith(", 2>(s2v::ConvArgs)") or ops.plan_symbol(p3).startswith(
        "void s2v::conv_x3_halo<2, "), ops.plan_symbol(p3)


def test_plan_symbols_of_the_mode():
    rc, pl, _ = _plan(16, 12, 12, 1024, 256)
    assert rc == 0 and ops.plan_symbol(pl).startswith("void s2v::conv_igemm_x3<") and \
        ops.plan_symbol(pl).endswith(", 2>(s2v::ConvArgs)"), ops.plan_symbol(pl)
    rc, pl, _ = _plan(4, 512, 512, 128, 64, in_scale=True)
    assert rc == 0 and ops.plan_symbol(pl) == "void s2v::conv_x3_halo<2, 4, 1>(s2v::ConvArgs)"
    rc, pl, _ = _plan(4, 256, 256, 128, 128)
    assert rc == 0 and ops.plan_symbol(pl) == "void s2v::conv_x3_halo<2, 4, 2>(s2v::ConvArgs)"


def test_fallback_families_report_the_precision_they_run():
    """conv_x3_nar (forced tiles 16 / 17), conv_head_x3 (a 7x7 64 -> 3 head) and x_split inputs (conv_glds_x3) have no
    single-pass instance: the plan of an "f16" launch is the f16x3 plan, out[6] == 2 included."""
    for kw in (dict(args=(2, 32, 32, 64, 64), force_tile=16), dict(args=(2, 32, 32, 64, 64), force_tile=17),
               dict(args=(1, 64, 64, 64, 3), k=7, pad=3), dict(args=(4, 64, 64, 64, 128), x_split=1)):
        args = kw.pop("args")
        rc3, p3, ws3 = _plan(*args, prec=3, **kw)
        rc2, p2, ws2 = _plan(*args, prec=2, **kw)
        assert rc3 == 0 and rc2 == 0, _lib.load().s2v_last_error()
        assert p3 == p2 and p3[6] == 2 and ws3 == ws2, (kw, p2, p3)
    rc, pl, _ = _plan(2, 32, 32, 64, 64, force_tile=16)
    assert ops.plan_symbol(pl) == "void s2v::conv_x3_nar<1, 0>(s2v::ConvArgs)"
    rc, pl, _ = _plan(1, 64, 64, 64, 3, k=7, pad=3)
    assert ops.plan_symbol(pl).startswith("void s2v::conv_head_x3<1, 3, 7,"), ops.plan_symbol(pl)
    rc, pl, _ = _plan(4, 64, 64, 64, 128, x_split=1)
    assert ops.plan_symbol(pl).startswith("void s2v::conv_glds_x3<") and ops.plan_symbol(pl).endswith(", 1>(s2v::ConvArgs)")
    # the exact-fp32 kernels stay what they are in every mode (a 4-channel 3x3: conv_k4_mfma)
    rc3, p3, _ = _plan(2, 32, 32, 4, 64, prec=3)
    rc2, p2, _ = _plan(2, 32, 32, 4, 64, prec=2)
    assert rc3 == 0 and p3 == p2 and ops.plan_symbol(p3).startswith("void s2v::conv_k4_mfma<")


def test_other_precision_codes_are_still_rejected():
    lib = _lib.load()
    for bad in (4, -1, 7):
        rc, _, _ = _plan(2, 16, 16, 64, 64, prec=bad)
        assert rc != 0 and b"bad prec %d" % bad in lib.s2v_last_error(), lib.s2v_last_error()


def test_group_plan_accepts_the_mode():
    """s2v_conv2d_group_plan answers the f16x3 grouping (tile and per-member splits) for prec 3, and still
    refuses members of two precisions."""
    lib = _lib.load()

    def member(prec, cin, cout, k):
        p = _lib.ConvParams()
        p.x, p.y, p.wt_x3, p.wt = 1 << 20, 2 << 20, 3 << 20, 4 << 20
        p.n, p.h, p.w, p.cin, p.xcs = 2, 14, 14, cin, cin
        p.kh = p.kw = k
        p.sh = p.sw = p.dh = p.dw = 1
        p.oh = p.ow = 14 - k + 1
        p.cout, p.ycs = cout, cout
        p.kpad, p.npad = (k * k * cin + 31) // 32 * 32, (cout + 127) // 128 * 128
        p.prec, p.batch = prec, 1
        return p
    plans = {}
    for prec in (2, 3):
        arr = (_lib.ConvParams * 2)(member(prec, 256, 64, 3), member(prec, 64, 192, 3))
        out = (ctypes.c_int * 5)()
        assert lib.s2v_conv2d_group_plan(arr, 2, out) == 0, lib.s2v_last_error()
        plans[prec] = (list(out)[:3], lib.s2v_conv2d_group_ws_bytes(arr, 2))
    assert plans[2] == plans[3], plans
    arr = (_lib.ConvParams * 2)(member(3, 256, 64, 3), member(2, 64, 192, 3))
    assert lib.s2v_conv2d_group_plan(arr, 2, (ctypes.c_int * 5)()) != 0
    assert b"one precision" in lib.s2v_last_error()


def test_inference_cli_offers_the_mode():
    from s2v_amd import inference
    ap = inference.build_parser()
    base = ["--face", "a.npy", "--audio", "a.wav"]
    assert ap.parse_args(base).precision is None                     # default: leave ops.PRECISION alone
    assert ap.parse_args(base + ["--precision", "f16"]).precision == "f16"
    with pytest.raises(SystemExit):
        ap.parse_args(base + ["--precision", "f16x2"])
    with pytest.raises(ValueError, match="precision must be one of"):  # before anything is read or launched
        inference.run("missing.npy", "missing.wav", precision="tf32")
