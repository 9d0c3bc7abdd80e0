"""The f16x3 range guard, site by site: every split-2 store raises the context's flag when its clamp fires, and only then.

include/pmp.h promises that every kernel storing a split-2 tensor raises a per-context flag when a value beyond +-65504 is clamped, so the
call is re-run on the fp32 datapath.  The promise is kept by hand in each kernel epilogue; a site that clamps without raising the flag
returns wrong logits silently, and one that raises it without cause makes every call run twice.  oracle/range_cases.py over-drives ONE
tensor at a time with a function-preserving weight gain (the rest of the graph stays below 65504 / 4, tests/test_range_cases_cpu.py), and
this file requires, for each case, on real QT / synthetic MTT weights, Luma and Chroma, four edge blocks:
  1. fusion off, taps on, PMP_SAT_IGNORE, s_over: each over-driven tensor is either clamped to exactly 65504 (stored units), which needs
     the flag up, or stored unclamped in fp32 within its layers64 bound (or, in a run, below 65504 behind an earlier clamped tensor whose
     clamped values it read); the flag is up exactly when something was clamped.  Flag down and clamped is the bug; flag up with nothing
     clamped is a false alarm;
  2. fusion on (the LDS-resident sites of chain16.hip / rbfuse32.hip, which have no taps), PMP_SAT_ERROR: PMP_E_RANGE exactly when 1 raised
     the flag;
  3. the default policy, fusion on: one re-run exactly when 1 raised the flag, its logits bit-identical to the fp32 datapath and within TOL
     of the oracle on the gained weights; no re-run and within TOL otherwise;
  4. s_under (the same tensors at 0.97 x 65504), both fusion settings: no flag, no re-run, within TOL of the oracle.
Then one case per MTT segment with non-zero activation-scale exponents from a .pmpw manifest: the thresholds are in stored units
(true x 2^-E), so a site that compares true values fails step 4 there."""
import os
import shutil
import time

import numpy as np
import pytest
import torch

import gpu_rig
from oracle import layers64 as L, parity as Y, range_cases as R, taps as T

pytestmark = pytest.mark.gpu
TOL = 1e-3


def _tap(e, name):
    got = T.tap(e, name)
    assert got is not None, "no tap " + name
    return got[0][:, :got[1]]


_taps_on = T.taps_on


def _oracle(gw, comp, blocks):
    return Y.oracle_logits(comp, 22, *blocks, wbd=gw[1], wq=gw[0])


def _bound_ratio(e, comp, gw, blocks, out, name, exps):
    """max |gpu - ref64| / bound of tensor `name` (layers64, f16x3) from the GPU's own inputs of its launch."""
    luma = comp == "Luma"
    logits = {"q/head": torch.from_numpy(out[0].astype(np.float64))}
    for k in range(3):
        logits["bd/head%d" % k] = torch.from_numpy(np.stack([out[1][:, k], out[2][:, k]], 1).astype(np.float64))
    cache = {}

    def get(n):
        if n in logits:
            return logits[n]
        if n not in cache:
            cache[n] = torch.from_numpy(np.ascontiguousarray(_tap(e, n)))
        return cache[n]
    x = L.blocks64(luma, *blocks)
    gen = L.q_layers(get, gw[0], luma, x, "f16x3") if name.startswith("q/") else L.msbd_layers(get, gw[1], luma, x, "f16x3", exps)
    for lay in gen:
        if lay.name == name:
            return L.ratio(get(name), lay)
    raise KeyError(name)


def run_case(case, comp, blocks, e_over, e_under, gw_over, gw_under, e32, exps=(0, 0, 0, 0, 0), load_under=None):
    """Steps 1-4 of the module docstring on engines that hold the gained weights (s_over / s_under; load_under(): puts the s_under
    weights into e_under before step 4, when it is the s_over context).  -> (problems, table line)."""
    from pmp_vvc_tip2023_amd import _lib
    bad = []
    tag = "%s %s" % (comp, case.name)
    y, u, v = blocks

    def infer(e):
        return e.inference_pre_QBD(comp, 22, y, u, v)
    # 1. fusion off, taps, no policy
    e = e_over
    e.set_fusion(False)
    e.set_saturation_policy("ignore")
    _taps_on(e, True)
    try:
        e.clear_saturation()
        out1 = infer(e)
        flag = e.saturated()
        amaxes, clamped = [], []
        for n in case.run:                          # launch order
            if n == R.STEM_Q:                       # no tap: the joint case's attention inputs carry the same logits
                continue
            t = _tap(e, n)
            sg = R.segment(n)
            st = float(np.abs(t).max()) * 2.0 ** -(exps[sg] if sg is not None else 0)
            if n not in case.over:
                if not st < R.LIMIT:
                    bad.append("%s: %s is not over-driven but stored at %.6g" % (tag, n, st))
                continue
            amaxes.append("%s %.6g" % (n, st))
            if not np.isfinite(t).all():
                bad.append("%s: %s holds non-finite values" % (tag, n))
            elif st == R.LIMIT:                     # clamped: the flag must be up
                clamped.append(n)
                if not flag:
                    bad.append("%s: flag DOWN but %s clamped (stored amax %.6g): a split-2 store that does not report" % (tag, n, st))
            elif st > R.LIMIT:                      # stored in fp32: unclamped, and right
                r = _bound_ratio(e, comp, gw_over, blocks, out1, n, exps)
                if r > 1.0:
                    bad.append("%s: %s unclamped at %.6g but %.3g x its float64 bound" % (tag, n, st, r))
            elif not clamped:                       # below 65504 is right only behind a clamp earlier in the run (it read clamped input)
                bad.append("%s: %s stored at %.6g: neither clamped to 65504 nor over-driven (wrapped?)" % (tag, n, st))
        if flag and not clamped:
            bad.append("%s: flag up with nothing clamped (%s): a false alarm" % (tag, ", ".join(amaxes) or "no tap"))
    finally:
        _taps_on(e, False)
    # 2. fused, PMP_SAT_ERROR
    e.set_fusion(True)
    e.set_saturation_policy("error")
    e.clear_saturation()
    code = 0
    try:
        infer(e)
        e.synchronize()
    except _lib.PmpError as err:
        code = err.code
    if code != (-7 if flag else 0):
        bad.append("%s: fused call under PMP_SAT_ERROR returned %d, the unfused one %s the flag" % (tag, code, "raised" if flag else "did not raise"))
    # 3. fused, default policy
    e.set_saturation_policy("rerun")
    e.clear_saturation()
    r0 = e.saturation_reruns()
    out3 = infer(e)
    reran = e.saturation_reruns() - r0
    if reran != (1 if flag else 0) or e.saturated() != flag:
        bad.append("%s: %d re-runs, saturated %s (unfused flag %s)" % (tag, reran, e.saturated(), flag))
    ref = _oracle(gw_over, comp, blocks)
    err3 = R.logit_err(out3, ref, case, case.s_over)
    if err3 >= TOL:
        bad.append("%s: s_over logits off the oracle by %.3g" % (tag, err3))
    if flag:
        e32.load(comp, 22, q_weights=gw_over[0], msbd_weights=gw_over[1])
        o32 = infer(e32)
        if not all(np.array_equal(a, b) for a, b in zip(out3, o32)):
            bad.append("%s: the re-run's logits are not the fp32 datapath's" % tag)
    # 4. s_under, both fusion settings
    if load_under is not None:
        load_under()
    e = e_under
    e.set_saturation_policy("rerun")
    ref = _oracle(gw_under, comp, blocks)
    for fusion in (False, True):
        e.set_fusion(fusion)
        e.clear_saturation()
        r0 = e.saturation_reruns()
        out4 = infer(e)
        if e.saturated() or e.saturation_reruns() != r0:
            bad.append("%s: s_under (stored 0.97 x 65504), fusion %s: the flag fired - a site compares the wrong quantity" % (tag, fusion))
        err4 = R.logit_err(out4, ref, case, case.s_under)
        if err4 >= TOL:
            bad.append("%s: s_under, fusion %s: logits off the oracle by %.3g" % (tag, fusion, err4))
        e.clear_saturation()
    line = "%-8s %-34s over %-60s flag %-5s %s" % (comp, case.name, ", ".join(amaxes) or "(no tap)", flag, "re-run" if reran else "no re-run")
    return bad, line


@pytest.fixture(scope="module")
def engines():
    scales_off = lambda e: e.set_activation_scales(False)           # exponents of zero: stored = true value
    with gpu_rig.engine("f16x3", synthetic_mtt=True, threads=16, setup=scales_off) as e16, gpu_rig.engine("fp32", synthetic_mtt=True) as e32:
        yield e16, e32


@pytest.mark.parametrize("comp", ["Luma", "Chroma"])
def test_every_split2_site_raises_the_flag_exactly_when_it_clamps(engines, comp):
    e16, e32 = engines
    t0 = time.time()
    print()
    blocks = R.gpu_blocks()
    cases, base, (wq, wb), _ = R.cases_for(comp)
    bad = []
    for case in cases:
        gw_over, gw_under = case.apply(wq, wb, case.s_over), case.apply(wq, wb, case.s_under)
        e16.load(comp, 22, q_weights=gw_over[0], msbd_weights=gw_over[1])
        b, line = run_case(case, comp, blocks, e16, e16, gw_over, gw_under, e32,
                           load_under=lambda: e16.load(comp, 22, q_weights=gw_under[0], msbd_weights=gw_under[1]))
        bad += b
        print(line)
    print("%s: %d cases in %.1f s" % (comp, len(cases), time.time() - t0))
    assert not bad, "\n".join(bad)


def test_segment_thresholds_are_in_stored_units(tmp_path):
    """One case per MTT segment with exponents (3, 2, 4, 3, 5) from the .pmpw manifest (activation scales on, no calibration pass): the
    over-driven tensor's stored value (true x 2^-E) brackets 65504, while its TRUE value at s_under is beyond 65504 x 2^(E-1)."""
    from pmp_vvc_tip2023_amd import engine, weights as W
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    blocks = R.gpu_blocks()
    cases, base, (wq, wb), _ = R.cases_for("Luma")
    seg = R.segment_cases(cases, base)
    e32 = engine.Engine(0)
    e32.set_precision("fp32")
    bad = []
    print()
    try:
        for k, case in enumerate(seg):
            eng = {}
            gws = {}
            for which, s in (("over", case.s_over), ("under", case.s_under)):
                gws[which] = case.apply(wq, wb, s)
                d = tmp_path / ("%d_%s" % (k, which))
                d.mkdir()
                shutil.copy(os.path.join(W.default_weight_dir(), "Luma_Q_22.pmpw"), d)
                W.save_pmpw(str(d / "Luma_BD_22.pmpw"), "Luma_MSBD", 22, gws[which][1], source="test", act_exp=R.SEGMENT_EXPS,
                            qt_partner=gws[which][0])
                e = engine.Engine(0, weight_dir=str(d))
                eng[which] = e
                e.load("Luma", 22)
                rep = e.activation_report("Luma", 22)
                assert rep["exps"] == list(R.SEGMENT_EXPS) and rep["tensors"] == [], (case.name, rep["exps"], len(rep["tensors"]))
            try:
                b, line = run_case(case, "Luma", blocks, eng["over"], eng["under"], gws["over"], gws["under"], e32, exps=R.SEGMENT_EXPS)
            finally:
                for e in eng.values():
                    e.close()
            bad += b
            print(line)
    finally:
        e32.close()
    assert not bad, "\n".join(bad)
