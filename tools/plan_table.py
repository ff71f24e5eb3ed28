#!/usr/bin/env python3
"""Every conv launch of an engine forward with the plan libs2v's planner picks for it, on the CPU.

The engine runs with torch.ops.s2v replaced by a stand-in whose conv ops fill an s2v_conv_params from
their arguments (the same fields csrc/torch_launch.cpp fills) and call the host-only
s2v_conv2d_plan of the in-tree libs2v.so (the device CU count falls back to 256 without a GPU); every
other op is a no-op.  Nothing is computed.

    python tools/plan_table.py lnet|enet|dnet|gfpgan|gpen|parsenet|lnet_fused [--batch 16]

``--record FILE`` writes the planner's decisions as a JSON fixture (tests/golden/conv_plans.json, replayed by
tests/test_host.py::test_planner_decisions_are_pinned): every conv / modconv / gemm / group launch of every engine
above at batch 1, 2 and 16, de-duplicated, and a deterministic synthetic sweep over the corners the engines do not
reach (sweep()).  ``--replay FILE`` runs a fixture's launches through the built library and prints, per launch, the
recorded and the current answer as JSON.  Both run with every S2V_* variable removed from the environment (the knobs are read once per process).

    python tools/plan_table.py --record tests/golden/conv_plans.json
"""
import argparse
import ctypes
import json
import os
import sys
from collections import Counter

if "--record" in sys.argv or "--replay" in sys.argv:
    for _k in [k for k in os.environ if k.startswith("S2V_")]:
        del os.environ[_k]

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402

import s2v_import  # noqa: E402,F401
from s2v_amd import _lib, ops  # noqa: E402


def _nv(t, step=1):
    n, h, w, c = t.shape
    return n, h, w, c, t.stride(2) // step, t.stride(0)


ENGINES = ("lnet", "enet", "dnet", "gfpgan", "gpen", "parsenet", "lnet_fused")
_PTR_FIELDS = {n for n, t in _lib.ConvParams._fields_ if t is ctypes.c_void_p}
# the twelve kernel families a plan (s2v_conv2d_plan's eleven ints) can name
ROUTES = ("glds", "head_x3", "halo_small", "small_cpar", "direct_small", "k4", "smallk", "smallk4", "x3_tile",
          "x3_nar", "x3_halo", "igemm")


def plan_route(out):
    bm, bn, wm, avec, code = out[:5]
    if avec == 5:
        return "glds"
    if avec in (6, 7):
        return "x3_nar"
    if avec == 8:
        return "x3_halo"
    if bm == 0:
        if wm < 0:
            return "smallk4" if code >= 2000 else "smallk"
        if code >= 1000:
            return {4: "k4", 3: "head_x3", 1: "halo_small"}[code // 1000]
        return "small_cpar" if wm else "direct_small"
    return "x3_tile" if out[6] else "igemm"


def params_record(p, align):
    """Every non-zero field of an s2v_conv_params; pointers as fake addresses that keep the pointer's value modulo
    256 (``align``: alignment drives routing) and which fields share one pointer (res == y)."""
    rec, fake = {}, {}
    for name, _ in _lib.ConvParams._fields_:
        v = getattr(p, name)
        if not v:
            continue
        if name in _PTR_FIELDS:
            v = fake.setdefault(v, 0x1000 * (len(fake) + 1) + align.get(v, v % 256))
        rec[name] = v
    return rec


def params_from(rec):
    p = _lib.ConvParams()
    for k, v in rec.items():
        setattr(p, k, v)
    return p


def answer(lib, rec):
    """What the planner says about one recorded launch (a field dict) or group (a list of them)."""
    if isinstance(rec, list):
        arr = (_lib.ConvParams * len(rec))(*[params_from(r) for r in rec])
        out = (ctypes.c_int * 5)()
        rc = lib.s2v_conv2d_group_plan(arr, len(rec), out)
        res = {"rc": rc, "out": list(out)[:1 + len(rec)] if rc == 0 else [], "ws": lib.s2v_conv2d_group_ws_bytes(arr, len(rec))}
    else:
        p = params_from(rec)
        out = (ctypes.c_int * 11)()
        rc = lib.s2v_conv2d_plan(ctypes.byref(p), out)
        res = {"rc": rc, "out": list(out) if rc == 0 else [], "ws": lib.s2v_conv2d_ws_bytes(ctypes.byref(p))}
    if rc:
        res["err"] = lib.s2v_last_error().decode()
    return res


class PlanOps:
    def __init__(self, lib):
        self.lib = lib
        self.rows = []
        self.launches = []      # params_record of every conv launch, a list of them for a group
        self.align = {}         # address -> its value modulo 256 on the device
        from s2v_amd import torch_ops
        self.ns = torch_ops.load()

    def ptr(self, t):
        """t's address; remembers the byte offset in its storage modulo 256, which is the address modulo 256 on the
        device, where every allocation is at least 256-byte aligned (the host allocator's 64-byte phase is noise)."""
        self.align[t.data_ptr()] = (t.data_ptr() - t.untyped_storage().data_ptr()) % 256
        return t.data_ptr()

    group = None

    def group_begin_(self):
        self.group = []

    def group_abort_(self):
        self.group = None

    def group_end_(self, ws, dry):
        members, self.group = self.group, None
        arr = (_lib.ConvParams * len(members))(*[p for p, _ in members])
        self.launches.append([params_record(p, self.align) for p, _ in members])
        out = (ctypes.c_int * 5)()
        rc = self.lib.s2v_conv2d_group_plan(arr, len(members), out)
        if rc:
            self.rows.append(("group!", tuple(e for _, e in members), [0] * 11))
        else:
            self.rows.append(("group", tuple(e[:7] for _, e in members), [out[0] + 1] + list(out)[1:1 + len(members)]))
        return [0, 0 if rc else 1]

    def _plan(self, p, what, extra):
        out = (ctypes.c_int * 11)()
        rc = self.lib.s2v_conv2d_plan(ctypes.byref(p), out)
        self.launches.append(params_record(p, self.align))
        if rc:
            raise RuntimeError(f"{what}: {ops._lib.load().s2v_last_error().decode()}")
        plan = list(out)
        if self.group is not None:
            self.group.append((p, extra))
            return [0] + plan
        self.rows.append((what, extra, plan))
        return [0] + plan

    def conv2d_(self, x, y, wt, wt_split, wt_scale, cout, kernel, stride, padding, dilation, in_mode, pad_mode, prec,
                scale, shift, in_scale, nc_scale, pre_act, pre_alpha, pix_add, pix_w, res, res_offset, res_after,
                act, alpha, out_step, out_pool, x_split, ws, grid_cap, force_tile, force_splits, *rest,
                post_mul=None, post_add=None, post_c0=0, dup_src=None, dup_bias=None, dup_a=0.0, dup_off=0):
        p = _lib.ConvParams()
        n, h, w, c, xcs, _ = _nv(x)
        yn, yh, yw, yc, ycs, _ = _nv(y, out_step)
        p.x, p.n, p.h, p.w, p.cin, p.xcs = self.ptr(x), n, h, w, c, xcs
        p.in_mode, p.pad_mode, p.pre_act = in_mode, pad_mode, pre_act
        p.in_scale = self.ptr(in_scale) if in_scale is not None else None
        p.in_scale_ns = in_scale.stride(0) if in_scale is not None else 0
        p.kh, p.kw = kernel
        p.sh, p.sw = stride
        p.ph, p.pw = padding
        p.dh, p.dw = dilation
        p.wt, p.npad, p.kpad, p.cout = self.ptr(wt), wt.shape[0], wt.shape[1], cout
        f = 2 if out_pool else 1
        p.y, p.oh, p.ow, p.ycs = self.ptr(y), yh * f, yw * f, ycs
        if out_step > 1:
            p.out_step, p.out_full_h, p.out_full_w = out_step, yh * out_step, yw * out_step
        p.nc_scale = self.ptr(nc_scale) if nc_scale is not None else None
        p.pix_add = self.ptr(pix_add) if pix_add is not None else None
        if res is not None:
            _, rh, rw, _, rcs, _ = _nv(res, out_step)
            p.res, p.res_cs, p.res_h, p.res_w = self.ptr(res), rcs, rh, rw
        p.act, p.batch, p.out_pool, p.x_split, p.prec = act, 1, int(out_pool), int(x_split), prec
        p.force_tile, p.force_splits, p.grid_cap = force_tile, force_splits, grid_cap
        p.wt_x3 = self.ptr(wt) if prec else None
        if post_mul is not None:
            p.post_mul, p.post_add, p.post_cs, p.post_c0 = self.ptr(post_mul), self.ptr(post_add), post_mul.stride(2), post_c0
        if dup_src is not None:
            p.dup_src, p.dup_cs, p.dup_a, p.dup_off = self.ptr(dup_src), dup_src.stride(2), dup_a, dup_off
            p.dup_bias = self.ptr(dup_bias) if dup_bias is not None else None
        return self._plan(p, "conv",(n, h, w, c, yh * f, yw * f, cout, p.kh, p.kw, grid_cap))

    def modulated_conv2d_(self, x, y, wt, s, d, wbuf, cout, kernel, padding, in_mode, prec, x_split, scale, shift,
                          pix_add, pix_w, res, res_after, act, alpha, ws, force_splits, st0, st1, st2, x_scale, flag,
                          dry, d2s=0, force_tile=0, *rest, **kw):
        p = _lib.ConvParams()
        n, h, w, c, xcs, xns = _nv(x)
        p.x, p.n, p.h, p.w, p.cin, p.xcs = self.ptr(x), 1, h, w, c, xcs
        p.batch, p.x_bs = n, xns
        p.in_mode = in_mode
        p.kh, p.kw = kernel
        p.sh = p.sw = p.dh = p.dw = 1
        p.ph, p.pw = padding
        p.wt, p.npad, p.kpad, p.cout = self.ptr(wbuf), wt.shape[0], wt.shape[1], cout
        p.w_bs = wt.shape[0] * wt.shape[1]
        if d2s:
            oh, ow = y.shape[1] // 2, y.shape[2] // 2
            p.out_step, p.out_full_h, p.out_full_w, p.d2s_cout = 2, y.shape[1], y.shape[2], cout // 4
            p.ycs = y.stride(2)
        else:
            oh, ow = y.shape[1], y.shape[2]
            p.ycs = y.stride(2)
        p.y, p.oh, p.ow = self.ptr(y), oh, ow
        p.pix_add = self.ptr(pix_add) if pix_add is not None else None
        if res is not None:
            p.res, p.res_cs, p.res_h, p.res_w = self.ptr(res), res.stride(2), res.shape[1], res.shape[2]
        p.act, p.prec, p.x_split, p.force_splits, p.force_tile = act, prec, int(x_split), force_splits, force_tile
        p.wt_x3 = self.ptr(wbuf) if prec else None
        return self._plan(p, "modconv", (n, h, w, c, oh, ow, cout, p.kh, p.kw, 0))

    def gemm_kn_(self, a, b, out, batch, a_bs, b_bs, out_bs, res, res_bs, act, alpha, prec, ws, force_tile,
                 force_splits, dry, *rest, **kw):
        p = _lib.ConvParams()
        M, K, N = a.shape[-2], a.shape[-1], b.shape[-1]
        p.x, p.n, p.h, p.w, p.cin, p.xcs = self.ptr(a), 1, 1, M, K, K
        p.kh = p.kw = p.sh = p.sw = p.dh = p.dw = 1
        p.wt, p.cout, p.b_kn, p.ldb, p.prec = self.ptr(b), N, 1, N, prec
        p.y, p.oh, p.ow, p.ycs = self.ptr(out), 1, M, N
        p.batch, p.x_bs, p.w_bs, p.y_bs = batch, a_bs, b_bs, out_bs
        p.force_tile, p.force_splits = force_tile, force_splits
        return self._plan(p, "gemm", (batch, 1, M, K, 1, M, N, 1, 1, 0))

    def __getattr__(self, name):
        schema = getattr(self.ns, name).default._schema
        ret = str(schema.returns[0].type) if schema.returns else ""

        def fn(*a):
            return [0] * 12 if ret.startswith("List") else 0 if ret == "int" else None
        return fn


def run(which, batch, po=None):
    from helpers import parsenet_sd, synth_sd
    from s2v_amd import synth
    lib = _lib.load()
    po = po or PlanOps(lib)
    ops.S2V = po
    ops._require_cuda = lambda t, what: None
    ctx = ops.Ctx("cpu")
    if which in ("lnet", "lnet_fused"):
        from s2v_amd.engine import lnet
        prev = lnet.FUSED, lnet.FUSED_LEVELS
        if which == "lnet_fused":
            lnet.FUSED, lnet.FUSED_LEVELS = True, (12, 24, 48)
        try:
            eng = lnet.LNetEngine(synth_sd("lnet"), "cpu")
            face6 = ops.NHWC(torch.zeros(batch, 96, 96, 6))
            eng.forward(ctx, torch.zeros(batch, 1, 80, 16), face6, ops.NHWC(torch.zeros(batch, 96, 96, 4)), pad_rgb=True)
        finally:
            lnet.FUSED, lnet.FUSED_LEVELS = prev
    elif which == "enet":
        from s2v_amd.engine.enet import ENetEngine
        eng = ENetEngine(synth_sd("enet"), "cpu")
        eng.forward(ctx, torch.zeros(batch, 1, 80, 16), torch.zeros(batch, 6, 256, 256), torch.zeros(batch, 3, 256, 256),
                    torch.empty(batch, 3, 384, 384), torch.empty(batch, 3, 96, 96))
    elif which == "dnet":
        from s2v_amd.engine.dnet import DNetEngine
        eng = DNetEngine(synth_sd("dnet"), "cpu")
        eng.forward(ctx, torch.zeros(batch, 3, 256, 256), torch.zeros(batch, 73, 26))
    elif which == "gfpgan":
        from s2v_amd.engine.gfpgan import GFPGANEngine
        eng = GFPGANEngine(synth_sd("gfpgan"), "cpu")
        x = torch.zeros(batch, 3, 512, 512)
        eng.forward(ctx, x, torch.empty_like(x), return_rgb=True, randomize_noise=True)
    elif which == "gpen":
        from s2v_amd.engine.gpen import GPENEngine
        eng = GPENEngine(synth_sd("gpen"), "cpu")
        x = torch.zeros(batch, 3, 512, 512)
        eng.forward(ctx, x, torch.empty_like(x))
    elif which == "parsenet":
        from s2v_amd.engine.parsenet import ParseNetEngine
        from s2v_amd.models.parse_arch import ParseNetParams, face_parse_net
        eng = ParseNetEngine(parsenet_sd(512), "cpu", ParseNetParams(**face_parse_net(512)).describe())
        eng.forward(ctx, torch.zeros(batch, 3, 512, 512), torch.empty(batch, 19, 512, 512), torch.empty(batch, 3, 512, 512))
    return po.rows


def _conv(prec, n, h, w, cin, cout, k, **kw):
    """A stride-1 'same' conv as the wrappers fill it: fake 256-byte aligned pointers, packed weights."""
    r = dict(x=0x1000, n=n, h=h, w=w, cin=cin, xcs=cin, kh=k, kw=k, sh=1, sw=1, ph=k // 2, pw=k // 2, dh=1, dw=1,
             wt=0x2000, kpad=(k * k * cin + 31) // 32 * 32, npad=(cout + 127) // 128 * 128, cout=cout,
             y=0x3000, oh=h, ow=w, ycs=cout, batch=1, prec=prec)
    if prec:
        r["wt_x3"] = 0x2000
    r.update(kw)
    return {k_: v for k_, v in r.items() if v}


# the shapes that reach each kernel family once: (prec, n, h, w, cin, cout, k, extra fields); prec 2 = f16x3
ROUTE_SHAPES = (
    (0, 2, 8, 8, 32, 64, 3, {}), (0, 2, 8, 8, 12, 64, 3, {}), (0, 2, 8, 8, 10, 64, 3, {}),
    (2, 2, 8, 8, 32, 64, 3, {}), (2, 2, 8, 8, 12, 64, 3, {}), (2, 2, 8, 8, 32, 64, 3, dict(pad_mode=1)),
    (2, 1, 8, 8, 256, 64, 3, {}), (2, 2, 8, 8, 32, 64, 3, dict(force_tile=16)), (2, 2, 8, 8, 32, 64, 3, dict(force_tile=17)),
    (2, 8, 256, 64, 32, 64, 3, {}), (2, 2, 256, 64, 32, 64, 3, {}), (2, 8, 256, 64, 32, 128, 3, {}),
    (2, 1, 8, 64, 32, 64, 3, dict(force_tile=19)), (2, 1, 9, 30, 32, 3, 7, {}), (2, 1, 9, 30, 128, 2, 5, {}),
    (0, 1, 9, 30, 64, 3, 7, {}), (2, 1, 9, 30, 8, 3, 3, {}), (2, 1, 9, 10, 128, 3, 1, {}), (2, 1, 9, 10, 32, 3, 1, {}),
    (2, 1, 9, 10, 2048, 3, 1, {}), (2, 1, 9, 10, 3, 1, 3, {}), (2, 1, 9, 10, 4, 32, 3, {}), (2, 1, 9, 10, 4, 64, 1, {}),
    (2, 1, 9, 10, 4, 16, 1, {}), (0, 1, 9, 10, 4, 16, 3, {}), (2, 1, 9, 10, 4, 512, 1, {}), (2, 1, 9, 10, 8, 16, 1, {}),
    (2, 4, 64, 64, 64, 256, 3, dict(force_tile=1, grid_cap=8)),
)


def sweep():
    """Deterministic synthetic launches over the corners the engines do not reach, illegal ones included."""
    recs = [_conv(*s[:7], **s[7]) for s in ROUTE_SHAPES]
    for prec in (0, 1, 2):
        ntiles = 6 if prec == 0 else 20
        recs += [_conv(prec, *s[1:7], **s[7]) for s in ROUTE_SHAPES if s[0] != prec and "force_tile" not in s[7]]
        # every force_tile of the precision's table and one past it, with force_splits 0 / 1 / 3
        for ft in range(1, ntiles + 2):
            for fs in (0, 1, 3):
                recs.append(_conv(prec, 2, 8, 8, 32, 64, 3, force_tile=ft, force_splits=fs))
            recs.append(_conv(prec, 1, 16, 64, 64, 128, 3, force_tile=ft))
            recs.append(_conv(prec, 1, 1, 40, 96, 48, 1, force_tile=ft, b_kn=1, ldb=48, kpad=0, npad=0, wt_x3=0))
        # filter sizes x channel counts at a small image
        for k in (1, 3, 5, 7):
            for cin in (3, 4, 8, 12, 32, 48, 64, 256):
                for cout in (1, 3, 4, 16, 32, 64, 96, 128, 256, 512):
                    if k >= 5 and (cout not in (1, 3, 4, 64) or cin in (12, 48)):
                        continue
                    recs.append(_conv(prec, 1, 9, 10, cin, cout, k))
        for cin, cout in ((32, 64), (64, 3), (4, 16)):
            base = (prec, 2, 8, 8, cin, cout, 3)
            recs += [
                _conv(*base, force_splits=1), _conv(*base, force_splits=3),
                _conv(prec, 1, 1, 40, cin, cout, 1, b_kn=1, ldb=(cout + 3) // 4 * 4, kpad=0, npad=0, wt_x3=0),
                _conv(prec, 1, 1, 40, cin, cout, 1, b_kn=1, ldb=(cout + 3) // 4 * 4, kpad=0, npad=0, wt_x3=0, batch=4,
                      x_bs=40 * cin, w_bs=cin * cout, y_bs=40 * cout),
                _conv(*base, x_split=1), _conv(prec, 4, 64, 64, cin, cout, 3, x_split=1),
                _conv(*base, out_pool=1), _conv(*base, out_pool=1, force_splits=3),
                _conv(prec, 4, 64, 64, cin, cout, 3, grid_cap=8), _conv(prec, 4, 64, 64, cin, cout, 3, grid_cap=64),
                _conv(prec, 1, 8, 8, cin, cout, 3, batch=2, x_bs=64 * cin, w_bs=128 * ((9 * cin + 31) // 32 * 32), y_bs=64 * cout),
                _conv(prec, 1, 16, 16, cin, cout, 3, batch=2, x_bs=256 * cin, w_bs=128 * ((9 * cin + 31) // 32 * 32),
                      y_bs=256 * cout),
                _conv(*base, in_scale=0x4000, in_scale_ns=cin), _conv(*base, in_scale=0x4004, in_scale_ns=cin),
                _conv(*base, pre_act=2, pre_alpha=0.2), _conv(*base, pre_act=3),
                _conv(*base, pad_mode=1), _conv(*base, pad_mode=1, ph=8, pw=8),
                _conv(*base, in_mode=1, oh=16, ow=16), _conv(*base, in_mode=1, oh=16, ow=16, pad_mode=1),
                _conv(*base, in_mode=2, sh=2, sw=2, oh=16, ow=16), _conv(*base, in_mode=2, pad_mode=1),
                _conv(*base, sh=2, sw=2, oh=4, ow=4), _conv(*base, dh=2, dw=2, ph=2, pw=2),
                _conv(*base, x=0x1004), _conv(*base, x=0x1004, force_tile=16),
                _conv(*base, force_tile=1), _conv(*base, force_tile=2, npad=0), _conv(*base, kpad=16),
                _conv(*base, out_step=2, out_full_h=16, out_full_w=16), _conv(*base, d2s_cout=cout // 4, out_step=2,
                                                                              out_full_h=16, out_full_w=16),
                _conv(*base, res=0x5000, res_cs=cout), _conv(*base, nc_scale=0x6000, nc_scale_ns=cout),
                _conv(*base, post_mul=0x7000, post_add=0x8000, post_cs=cout, post_c0=0),
            ]
    return recs


_CLASS_FIELDS = ("kh", "kw", "sh", "sw", "ph", "pw", "dh", "dw", "prec", "batch", "in_mode", "pad_mode", "cin", "cout")


def pack(pairs, answers, by=_CLASS_FIELDS):
    """(fields, answer) pairs -> classes {"const", "fields", "rows"}: launches with the same non-zero fields and
    the same values of the ``by`` fields share one class; a row holds the fields that vary inside it, then the
    position of its answer [rc, ws, out11... or the error text] in ``answers`` (appended to as needed)."""
    classes = {}
    for rec, ans in pairs:
        key = (tuple(rec), tuple(rec.get(f, 0) for f in by))
        classes.setdefault(key, []).append((rec, ans))
    out = []
    for (names, _), members in classes.items():
        const = {f: members[0][0][f] for f in names if all(r[f] == members[0][0][f] for r, _ in members)}
        fields = [f for f in names if f not in const]
        rows = []
        for r, a in members:
            ans = [a["rc"], a["ws"]] + (a["out"] if a["rc"] == 0 else [a["err"]])
            if ans not in answers:
                answers.append(ans)
            rows.append([r[f] for f in fields] + [answers.index(ans)])
        out.append({"const": const, "fields": fields, "rows": rows})
    return out


def unpack(classes, answers):
    """The (fields, answer) pairs of pack(), in file order."""
    pairs = []
    for c in classes:
        order = [n for n, _ in _lib.ConvParams._fields_]
        for row in c["rows"]:
            rec = dict(c["const"], **dict(zip(c["fields"], row[:-1])))
            a = answers[row[-1]]
            ans = {"rc": a[0], "ws": a[1], "out": a[2:] if a[0] == 0 else []}
            if a[0]:
                ans["err"] = a[2]
            pairs.append(({f: rec[f] for f in order if f in rec}, ans))
    return pairs


def load_fixture(path):
    """{"engines": pairs, "sweep": pairs, "groups": (list of member fields, answer) pairs} of a recorded file."""
    with open(path) as f:
        doc = json.load(f)
    fx = {s: unpack(doc[s], doc["answers"]) for s in ("engines", "sweep")}
    fx["groups"] = [([fx["engines"][i][0] for i in g[:-1]], {"rc": g[-1][0], "ws": g[-1][1], "out": g[-1][2:]})
                    for g in doc["groups"]]
    return fx


def record(path):
    lib = _lib.load()
    assert lib.s2v_device_cus() in (0, 256), "record on a machine without a GPU or on a 256-CU device"
    seen, singles, groups = {}, {"engines": [], "sweep": []}, {}

    def add(section, rec):
        key = json.dumps(rec, sort_keys=True)
        if key not in seen:
            seen[key] = (section, len(singles[section]))
            singles[section].append((rec, answer(lib, rec)))
        return key
    for which in ENGINES:
        for batch in (1, 2, 16):
            po = PlanOps(lib)
            run(which, batch, po)
            for rec in po.launches:
                if isinstance(rec, list):
                    groups.setdefault(tuple(add("engines", m) for m in rec), rec)
                else:
                    add("engines", rec)
            print(f"{which} batch {batch}: {len(po.launches)} launches, {len(singles['engines'])} distinct so far", file=sys.stderr)
    for rec in sweep():
        add("sweep", rec)
    routes = Counter(plan_route(a["out"]) for s in singles.values() for _, a in s if a["rc"] == 0)
    assert set(routes) == set(ROUTES), sorted(set(ROUTES) - set(routes))
    doc = {"answers": []}
    doc["engines"] = pack(singles["engines"], doc["answers"])
    doc["sweep"] = pack(singles["sweep"], doc["answers"], by=("prec",))
    # a group: the positions of its members among the engine launches in file order, then the answer
    where = {json.dumps(r, sort_keys=True): i for i, (r, _) in enumerate(unpack(doc["engines"], doc["answers"]))}
    doc["groups"] = []
    for keys, members in groups.items():
        a = answer(lib, members)
        assert a["rc"] == 0, a
        doc["groups"].append([where[k] for k in keys] + [[a["rc"], a["ws"]] + a["out"]])

    def lines(items, per=1):        # one class per line, sixteen answers / groups per line
        text = [json.dumps(i, separators=(",", ":")) for i in items]
        return "[\n" + ",\n".join(",".join(text[i:i + per]) for i in range(0, len(text), per)) + "\n]"
    with open(path, "w") as f:
        f.write("{" + ",\n".join(f'"{s}": {lines(doc[s], 1 if s in ("engines", "sweep") else 16)}' for s in ("answers", "engines", "sweep", "groups")) + "}\n")
    print(f"{path}: {len(singles['engines'])} engine launches, {len(singles['sweep'])} sweep launches, {len(groups)} groups, "
          f"{os.path.getsize(path)} bytes; routes {dict(routes)}", file=sys.stderr)


def replay(path):
    """Per section, every launch of a fixture with the recorded answer ("want"), the library's ("got") and the kernel
    family the recorded plan names ("route"), as JSON on stdout."""
    lib = _lib.load()
    fx = load_fixture(path)
    json.dump({"cus": lib.s2v_device_cus(),
               **{s: [{"p": r, "want": a, "got": answer(lib, r),
                       "route": plan_route(a["out"]) if a["rc"] == 0 and isinstance(r, dict) else None} for r, a in fx[s]]
                  for s in ("engines", "sweep", "groups")}}, sys.stdout)


def dump_text(path, count):
    """Every (len / count)-th single launch of a fixture as a line "field=value ... | rc ws out..." (tools/plan_replay.cpp)."""
    fx = load_fixture(path)
    pairs = fx["engines"] + fx["sweep"]
    for rec, a in pairs[::max(1, len(pairs) // count)]:
        print(" ".join(f"{k}={v!r}" for k, v in rec.items()), "|", a["rc"], a["ws"], *a["out"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("which", choices=ENGINES, nargs="?")
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--record", metavar="FILE")
    ap.add_argument("--replay", metavar="FILE")
    ap.add_argument("--dump-text", metavar=("FILE", "COUNT"), nargs=2)
    a = ap.parse_args()
    if a.record:
        return record(a.record)
    if a.replay:
        return replay(a.replay)
    if a.dump_text:
        return dump_text(a.dump_text[0], int(a.dump_text[1]))
    if not a.which:
        ap.error("an engine, --record FILE or --replay FILE")
    rows = run(a.which, a.batch)
    syms = Counter()
    nsplit = 0
    for what, shp, plan in rows:
        if what.startswith("group"):
            print(f"{what:8s} members (n,h,w,cin,oh,ow,cout)={shp} x3 tile cfg (force_tile)={plan[0]} splits={plan[1:]}")
            syms[what + f" tile {plan[0]}"] += 1
            nsplit += any(v > 1 for v in plan[1:])
            continue
        sym = ops.plan_symbol(plan)
        syms[sym[10:60]] += 1
        nsplit += plan[5] > 1
        print(f"{what:8s} n,h,w,cin,oh,ow,cout,kh,kw,cap={shp} splits={plan[5]} {sym[10:70]}")
    print(f"{len(rows)} conv launches, {nsplit} with split-K (+{nsplit} reduce launches)")
    for k, v in syms.most_common():
        print(f"  {v:4d} {k}")


if __name__ == "__main__":
    main()
