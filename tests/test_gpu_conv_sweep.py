"""Every case of oracle/conv_cases.py - ResidualBlocks at shapes, weights and activations beyond the four nets - through the product code
(pmp_debug_run_resblock, include/pmp.h) on its datapath, each launch checked per element against the float64 bound of oracle/layers64.py
built from the kernel's own inputs (the taps), in poisoned workspaces (an unwritten pooled element or tile shows).  The f16x3 cases that
the fused 32x32 kernel accepts run fused and launch per layer, bit-identical.  The launched instantiations must be the ones the dispatch
table predicts, and together the table's reachable set; the f16x3 range flag stays clear on every case and rises for an output driven
just over 65504 * 2^E on every f16x3 instantiation.  `pytest -s` prints the worst ratio per instantiation and datapath."""
import collections
import ctypes as C
import time

import numpy as np
import pytest
import torch

import gpu_rig
from oracle import conv_cases as CC
from oracle import layers64 as L
from oracle import taps as T

pytestmark = pytest.mark.gpu

FIELDS = ("n", "h", "w", "cin", "cout", "k", "gate", "pool", "out_f32", "exp_x", "exp_gate", "exp_out")


class RBCase(C.Structure):
    _fields_ = [(f, C.c_int) for f in FIELDS]


def _fp(a):
    return None if a is None else np.ascontiguousarray(a, np.float32).ctypes.data_as(C.POINTER(C.c_float))


def run_block(e, c, x, w0, w2, wsc, gate):
    """-> (return code, range flag fired, launched instantiations)."""
    cs = RBCase(*[int(c.get(f, 0)) for f in FIELDS])
    sat, buf = C.c_int(-1), C.create_string_buffer(4096)
    keep = [np.ascontiguousarray(a, np.float32) if a is not None else None for a in (x, w0, w2, wsc, gate)]
    rc = e.lib.pmp_debug_run_resblock(e.h, C.byref(cs), *[_fp(a) for a in keep], C.byref(sat), buf, len(buf))
    return rc, sat.value, buf.value.decode().split()


# taps on; poison 2: finite garbage (0x3C bytes) before every pass
eng = gpu_rig.engine_fixture(threads=16, setup=lambda e: T.taps_on(e, True), poison=2)


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float64))


def check_case(e, c, x, w0, w2, wsc, gate, fusion=False):
    """Runs case c; -> (ratio .t or None, ratio out, out tap, flag, kernels).  The bound is built from the taps: what the kernels read."""
    e.set_precision(c["dp"])
    e.set_fusion(fusion)
    rc, sat, kern = run_block(e, c, x, w0, w2, wsc, gate)
    e._ck(rc)
    dp = c["dp"]
    xg = _t(T.tap(e, "x")[0])
    gg = _t(T.tap(e, "gate")[0]) if c["gate"] else None
    tt = T.tap(e, "rb.t")
    tt = (_t(tt[0]),) if tt is not None else None
    y = _t(T.tap(e, "rb")[0])
    E = (c["exp_x"], c["exp_out"]) if dp == "f16x3" else (0, 0)
    w0d, w2d, wscd = _t(w0), _t(w2), (_t(wsc.reshape(wsc.shape[0], -1, 1, 1)) if wsc is not None else None)
    rt = None
    if tt is not None:
        lay = L.Layer("rb.t", "", *L.conv_t64(xg, w0d, dp, E[0]))
        rt = L.ratio(tt[0], lay)
        t_in = tt[0]
    else:
        t_in = None
    return rt, t_in, y, sat, kern, (xg, gg, w0d, w2d, wscd, E)


def out_ratio(c, t_in, y, ins):
    xg, gg, w0d, w2d, wscd, E = ins
    lay = L.Layer("rb", "", *L.conv_out64(xg, t_in, w2d, wscd, c["dp"], gg, c["pool"], E[1]))
    return L.ratio(y, lay)


def test_refused_shapes_return_invalid(eng):
    x = np.ones(16 * 64 * 64 * 128, np.float32)
    for dp in CC.DATAPATHS:
        eng.set_precision(dp)
        for r in CC.REFUSED:
            c = dict(r)
            cin, cout, k = max(c["cin"], 1), max(c["cout"], 1), max(c["k"], 1)
            w0 = np.ones(cout * cin * k * k, np.float32)
            w2 = np.ones(cout * cout * k * k, np.float32)
            rc, _, kern = run_block(eng, c, x, w0, w2, np.ones(cout * cin, np.float32), x)
            assert rc == -1 and kern == [], (dp, r, rc, kern)
    # a gated identity-shortcut block whose gate product steps between activation scales: the step rides on the accumulator's out_scale,
    # which an identity residual would miss, so the graph refuses it (no block of the nets is such a block)
    c = dict(dp="f16x3", n=1, h=16, w=16, cin=16, cout=16, k=3, gate=1, exp_x=2, exp_gate=1, exp_out=0)
    eng.set_precision("f16x3")
    w = np.ones(16 * 16 * 9, np.float32) / 64
    rc, _, kern = run_block(eng, c, x, w, w, None, x)
    assert rc == -1 and kern == [], (rc, kern)


def test_conv_sweep_against_float64(eng):
    t0 = time.time()
    worst = collections.defaultdict(float)
    reached = set()
    fails = []
    cases = CC.cases()
    flag_base = {}                  # f16x3 instantiation -> a case whose launch of it we can drive over range
    for c in cases:
        x, w0, w2, wsc, gate = CC.tensors(c)
        rt, t_in, y, sat, kern, ins = check_case(eng, c, x, w0, w2, wsc, gate)
        want = CC.expected_kernels(c, fusion=False)
        if kern != want:
            fails.append("%s: launched %s, dispatch table says %s" % (c["id"], kern, want))
            continue
        reached.update(kern)
        ry = out_ratio(c, t_in, y, ins)
        worst[(kern[0], c["dp"])] = max(worst[(kern[0], c["dp"])], rt)
        worst[(kern[1], c["dp"])] = max(worst[(kern[1], c["dp"])], ry)
        if not (rt <= 1.0 and ry <= 1.0):
            fails.append("%s: max |gpu - ref64| / bound .t %.3g (%s), out %.3g (%s)" % (c["id"], rt, kern[0], ry, kern[1]))
        if sat:
            fails.append("%s: range flag raised in range" % c["id"])
        if CC.fused32(c):
            rf, _, yf, satf, kf, _ = check_case(eng, c, x, w0, w2, wsc, gate, fusion=True)
            reached.update(kf)
            if kf != CC.expected_kernels(c) or rf is not None or not torch.equal(yf, y) or satf:
                fails.append("%s: fused run (%s) not bit-identical to the launch-per-layer one" % (c["id"], kf))
        if c["dp"] == "f16x3" and c["xdist"] != "zero" and not c["wdist"].startswith("zero") and float(y.abs().max()) > 0:
            flag_base.setdefault(kern[0], (c, 0))                      # the first launch: no shortcut source
            if wsc is not None and not c["out_f32"]:
                flag_base.setdefault(kern[1], (c, 1))                  # the second with a 1x1 shortcut: its split-2 store
    # the range flag: each f16x3 instantiation's store driven to 1.02 (and 0.97) of 65504 * 2^E
    flags = {}
    for kname, (c, i) in sorted(flag_base.items()):
        x, w0, w2, wsc, gate = CC.tensors(c)
        _, t_in, y, _, _, _ = check_case(eng, c, x, w0, w2, wsc, gate)
        E = c["exp_x"] if i == 0 else c["exp_out"]
        top = float((t_in if i == 0 else y).abs().max())
        got = []
        for f in (1.02, 0.97):
            s = f * 65504.0 * 2.0 ** E / top
            if i == 0:      # .t over range, w2 shrunk by as much so that the output stays in range
                args = (x, w0 * np.float32(s), w2 / np.float32(s), wsc, gate)
            elif wsc is not None:
                args = (x, w0, w2 * np.float32(s), wsc * np.float32(s), gate)
            else:
                args = None
            if args is None:
                break
            _, _, _, sat, kern, _ = check_case(eng, c, *args)
            got.append(sat)
        if got:
            flags[kname] = got
            if got != [1, 0]:
                fails.append("%s via %s: range flag %s at 1.02 / 0.97 of 65504 * 2^E (want raised / clear)" % (kname, c["id"], got))
    h2 = {k for k in CC.INSTANTIATIONS if k.startswith("conv_h2")}
    missing = h2 - set(flags)
    print("\n%d cases in %.1f s; worst |gpu - ref64| / bound per instantiation and datapath:" % (len(cases), time.time() - t0))
    for (kname, dp), r in sorted(worst.items()):
        print("  %-34s %-7s %.3f" % (kname, dp, r))
    print("range flag at 1.02 / 0.97 of 65504 * 2^E:", " ".join("%s=%s" % kv for kv in sorted(flags.items())))
    print("reached:", " ".join(sorted(reached)))
    reachable = {k for k, v in CC.INSTANTIATIONS.items() if v is None} | set(CC.FUSED)
    assert not fails, "\n".join(fails[:40])
    assert reached == reachable, (sorted(reachable - reached), sorted(reached - reachable))
    assert not missing, "no range-flag case for %s" % sorted(missing)
