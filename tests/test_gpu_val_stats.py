"""GPU: validation statistics (include/pmp.h: pmp_val_stats, logitstats.hip) and teacher-forced MTT inference (pmp_infer_msbd).

Bounds.  The seven hit counts are integers: EXACT.  The thirteen sums: the kernel and the numpy restatement (tests/val_cases.py) add the
SAME float32 terms in float64, at most 2e5 of them, in different orders - 1e-12 relative covers any order (n * 2^-53 = 2.2e-11 is the
worst case of a serial sum; both sides are trees or short chains) - and therefore, by the triangle inequality, within ref_vs_f64 + 1e-12
of the reference's numbers, ref_vs_f64 being the reference-to-restatement distance the golden generator measured and stored in G12."""
import json
import os

import numpy as np
import pytest

from conftest import golden
import gpu_rig
import val_cases as K
from oracle import parity as Y

pytestmark = pytest.mark.gpu

SUM_TOL = 1e-12
TOL = 1e-3          # the project's logit tolerance against the oracle
MODES = (("qbd", "vqbd"), ("q", "pre0"), ("bd", "pre1"))

eng = gpu_rig.engine_fixture(synthetic_mtt=True)


@pytest.fixture(scope="module")
def g12():
    return golden("g12_val.npz")


def same(got, want, what=""):
    """Counts exact, sums within SUM_TOL (NaN / inf entries equal in kind)."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert np.array_equal(got[..., K.COUNTS], want[..., K.COUNTS]), (what, got[..., K.COUNTS], want[..., K.COUNTS])
    d = K.rel_dist(got[..., K.SUMS], want[..., K.SUMS])
    assert d <= SUM_TOL, (what, d)
    return d


def kw_of(c, s=slice(None), mode="qbd"):
    kw = {}
    if mode in ("qbd", "q"):
        kw.update(qt=c["qt"][s], qt8=c["qt8"][s])
    if mode in ("qbd", "bd"):
        kw.update(bt=c["bt"][s], dire=c["dire"][s], msbt=c["msbt"][s], msdire=c["msdire"][s])
    return kw


def dev_stats(e, qp, kw, block_stats=False):
    """pmp_val_stats_device on uploaded copies -> (S[20], per-block [n,20] or None)."""
    import torch
    order = ("qt", "bt", "dire", "qt8", "msbt", "msdire")
    d = {k: torch.from_numpy(np.ascontiguousarray(kw[k])).cuda() if k in kw else None for k in order}
    n = len(kw["qt"] if "qt" in kw else kw["bt"])
    S = torch.full((20,), -1.0, dtype=torch.float64, device="cuda")
    B = torch.full((n, 20), -1.0, dtype=torch.float64, device="cuda") if block_stats else None
    torch.cuda.synchronize()
    e.val_stats_device(qp, *[None if d[k] is None else d[k].data_ptr() for k in order], n, S.data_ptr(), None if B is None else B.data_ptr())
    e.synchronize()
    torch.cuda.synchronize()
    return S.cpu().numpy(), (None if B is None else B.cpu().numpy())


# ---- 1. every form against the restatement and, through it, the reference
@pytest.mark.parametrize("name", list(K.CASES))
def test_stats_equal_restatement_and_reference(eng, g12, name):
    c = K.make(name)
    ref_tol = float(g12["ref_vs_f64"]) + SUM_TOL
    for mode, key in MODES:
        want, ns = K.case_stats(c, mode)
        host = np.stack([eng.val_stats(c["qp"], **kw_of(c, slice(o, o + m), mode)) for o, m in K.batches(c)])
        dev = np.stack([dev_stats(eng, c["qp"], kw_of(c, slice(o, o + m), mode))[0] for o, m in K.batches(c)])
        print("%s %s: host vs restatement %.3g, device vs restatement %.3g" % (name, mode, same(host, want, "host"), same(dev, want, "device")))
        if mode == "q":
            assert not host[:, 1:13].any() and not host[:, 14:].any()
        if mode == "bd":
            assert not host[:, 0].any() and not host[:, 13].any()
        from pmp_vvc_tip2023_amd import engine
        for S in (host, dev):
            got = np.array(engine.validation_numbers(S, ns, mode))
            ref = g12["%s_%s" % (name, key)]
            assert np.array_equal(got[K.EXACT[mode]], ref[K.EXACT[mode]]), (name, mode)
            d = K.rel_dist(got, ref)
            print("%s %s: vs the reference %.3g (bound %.3g)" % (name, mode, d, ref_tol))
            assert d <= ref_tol, (name, mode, d)


def test_whole_call_chunks_empty_and_errors(eng):
    from pmp_vvc_tip2023_amd import _lib
    c = K.make("qp37")
    want = K.stats(37, **kw_of(c))
    s0 = eng.val_stats(37, **kw_of(c))
    same(s0, want, "one pass")
    eng.set_chunk(64)                            # 450 blocks = 8 passes: other bits allowed, same counts, same bound
    try:
        s1 = eng.val_stats(37, **kw_of(c))
    finally:
        eng.set_chunk(4096)
    same(s1, want, "8 passes")
    assert np.array_equal(s0[K.COUNTS], s1[K.COUNTS])
    z = eng.val_stats(22, **kw_of(c, slice(0, 0)))
    assert z.shape == (20,) and not z.any()
    import torch
    S = torch.full((20,), 7.0, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    eng.val_stats_device(22, None, None, None, None, None, None, 0, S.data_ptr())
    eng.synchronize()
    assert not S.cpu().numpy().any()
    for qp in (21, 42, 0):
        with pytest.raises(_lib.PmpError) as ei:
            eng.val_stats(qp, **kw_of(c))
        assert ei.value.code == -1
    q = np.ascontiguousarray(c["qt"][:4]); b = np.ascontiguousarray(c["bt"][:4])
    out = np.zeros(20)
    P = lambda a: a.ctypes.data
    rc = eng.lib.pmp_val_stats(eng.h, 27, P(q), P(b), None, None, None, None, 4, P(out))       # a NULL mix
    assert rc == -1
    rc = eng.lib.pmp_val_stats(eng.h, 27, P(q), None, None, None, None, None, 4, P(out))       # logits without labels
    assert rc == -1
    d = torch.zeros(4 * 768 + 4, device="cuda")
    l8 = torch.zeros(4 * 768, dtype=torch.uint8, device="cuda")
    rc = eng.lib.pmp_val_stats_device(eng.h, 27, None, d.data_ptr() + 4, d.data_ptr(), None, l8.data_ptr(), l8.data_ptr(), 4, S.data_ptr(), None)
    assert rc == -1                               # bt not 16-byte aligned


# ---- 2. bit-reproducibility
def test_bits_do_not_depend_on_run_context_stream_or_block_output(eng):
    import torch
    from pmp_vvc_tip2023_amd import engine
    c = K.make("qp32")
    kw = kw_of(c)
    a, _ = dev_stats(eng, 32, kw)
    b, _ = dev_stats(eng, 32, kw)
    s, blk = dev_stats(eng, 32, kw, block_stats=True)
    assert a.tobytes() == b.tobytes() == s.tobytes()
    e2 = engine.Engine(0)
    try:
        d, blk2 = dev_stats(e2, 32, kw, block_stats=True)
    finally:
        e2.close()
    assert d.tobytes() == a.tobytes() and blk2.tobytes() == blk.tobytes()
    stream = torch.cuda.Stream()
    eng.set_stream(stream.cuda_stream)
    try:
        with torch.cuda.stream(stream):
            f, _ = dev_stats(eng, 32, kw)
    finally:
        eng.set_stream(None)
    assert f.tobytes() == a.tobytes()
    # the per-block partials: each block's own twenty numbers, and they add up to the batch in the documented order
    same(blk, K.block_stats(32, **kw), "per block")
    part = np.zeros((16, 20))
    for g in range(16):
        for row in blk[g::16]:
            part[g] += row
    tot = part[0].copy()
    for g in range(1, 16):
        tot += part[g]
    assert tot.tobytes() == a.tobytes()
    # the QT-only and MTT-only forms are the matching columns of the full form, bit for bit
    q, _ = dev_stats(eng, 32, kw_of(c, mode="q"))
    m, _ = dev_stats(eng, 32, kw_of(c, mode="bd"))
    assert q[[0, 13]].tobytes() == a[[0, 13]].tobytes() and np.delete(m, [0, 13]).tobytes() == np.delete(a, [0, 13]).tobytes()


# ---- 3. the engine's validation through batching, against the reference's numbers
@pytest.mark.parametrize("name", list(K.CASES))
def test_engine_validation_equals_reference_golden(eng, g12, name):
    c = K.make(name)
    ref_tol = float(g12["ref_vs_f64"]) + SUM_TOL
    for mode, key in MODES:
        logits = {"qbd": (c["qt"], c["bt"], c["dire"]), "q": (c["qt"],), "bd": (c["bt"], c["dire"])}[mode]
        if mode == "qbd":
            got, blk = eng.validation_QBD("Luma", c["qp"], None, c["qt8"], c["msbt"], c["msdire"], batch_size=c["batch"], logits=logits,
                                          return_block_stats=True)
            same(blk, K.block_stats(c["qp"], **kw_of(c)), "per block")
        else:
            got = eng.pre_validation("Luma", c["qp"], 0 if mode == "q" else 1, None, c["qt8"], c["msbt"], c["msdire"], batch_size=c["batch"],
                                     logits=logits)
        got, ref = np.array(got), g12["%s_%s" % (name, key)]
        assert got.shape == ref.shape
        assert np.array_equal(got[K.EXACT[mode]], ref[K.EXACT[mode]]), (name, mode)
        d = K.rel_dist(got, ref)
        print("%s %s: engine vs the reference %.3g (bound %.3g)" % (name, mode, d, ref_tol))
        assert d <= ref_tol
        mine, _ = K.numbers(*K.case_stats(c, mode), mode)
        assert K.rel_dist(got, mine) <= SUM_TOL
    # groups of batches smaller than the set: same numbers, bit for bit
    a = eng.validation_QBD("Luma", c["qp"], None, c["qt8"], c["msbt"], c["msdire"], batch_size=c["batch"], logits=(c["qt"], c["bt"], c["dire"]))
    from pmp_vvc_tip2023_amd import engine, validation
    r = validation.run(eng, "qbd", "Luma", c["qp"], None, c["qt8"], c["msbt"], c["msdire"], c["batch"], (c["qt"], c["bt"], c["dire"]),
                       group_blocks=c["batch"])
    assert np.array(engine.validation_numbers(r.S, r.ns)).tobytes() == np.array(a).tobytes()
    with pytest.raises(ValueError):
        eng.pre_validation("Luma", 22, 2, None, c["qt8"])


def test_batch_ranges_join_into_the_whole_run_in_every_mode(eng):
    """25 blocks at batch 10: a ragged last batch of 5, three groups at group_blocks=10, and the ranges (0,1), (1,3), (3,3) - the last an
    empty share - joined against the whole run, as bytes; no nets run."""
    import confusion_cases as X
    from pmp_vvc_tip2023_amd import validation as V
    c = {k: (v[:25] if isinstance(v, np.ndarray) else v) for k, v in K.make("qp41_small").items()}
    c.update(n=25, batch=10)
    lab = (c["qt8"], c["msbt"], c["msdire"])
    wholes = {}
    for mode in V.MODES:
        logits = {"qbd": (c["qt"], c["bt"], c["dire"]), "q": (c["qt"],), "bd": (c["bt"], c["dire"])}[mode]
        call = lambda **kw: V.run(eng, mode, "Luma", c["qp"], None, *lab, 10, logits, want_confusion=True, group_blocks=10, **kw)
        whole = wholes[mode] = call()
        assert whole.mode == mode and whole.ns == [10, 10, 5] and whole.S.shape == (3, 20) and whole.conf.shape == (3, 7, 5, 5)
        same(whole.S, K.case_stats(c, mode)[0], mode)
        for i, (o, m) in enumerate(K.batches(c)):
            assert np.array_equal(whole.conf[i], X.counts(**kw_of(c, slice(o, o + m), mode))), (mode, i)
        parts = [call(batch_range=r) for r in ((0, 1), (1, 3), (3, 3))]
        assert [p.ns for p in parts] == [[10], [10, 5], []] and parts[2].S.shape == (0, 20) and parts[2].conf.shape == (0, 7, 5, 5)
        j = V.ValRun.join(parts)
        assert j.ns == whole.ns and j.S.tobytes() == whole.S.tobytes() and j.conf.tobytes() == whole.conf.tobytes()
        assert np.array(j.numbers()).tobytes() == np.array(whole.numbers()).tobytes() and len(j.numbers()) == len(V.NAMES[mode])
    got, blk, conf = eng.validation_QBD("Luma", c["qp"], None, *lab, batch_size=10, logits=(c["qt"], c["bt"], c["dire"]), return_block_stats=True,
                                        return_confusion=True)
    w = V.run(eng, "qbd", "Luma", c["qp"], None, *lab, 10, (c["qt"], c["bt"], c["dire"]), want_blocks=True, want_confusion=True)
    assert np.array(got).tobytes() == np.array(w.numbers()).tobytes() == np.array(wholes["qbd"].numbers()).tobytes()
    assert blk.shape == (25, 20) and blk.tobytes() == w.block_stats.tobytes()
    assert conf.dtype == np.int64 and conf.tobytes() == w.confusion().tobytes() == wholes["qbd"].confusion().tobytes()


# ---- 4. teacher-forced MTT inference
def _infer_dev(e, comp, qp, y, u, v, qt_in=None):
    """pmp_infer_device (qt_in None) or pmp_infer_msbd_device -> (qt or None, bt, dire, qt_in after the call)."""
    import torch
    n = len(y)
    d = [torch.from_numpy(a).cuda() for a in ((y, u, v) if comp == "Chroma" else (y,))]
    p = [t.data_ptr() for t in d] + [None] * (3 - len(d))
    bt = torch.zeros((n, 3, 16, 16), device="cuda"); dire = torch.zeros((n, 3, 16, 16), device="cuda")
    if qt_in is None:
        qt = torch.zeros((n, 1, 8, 8), device="cuda")
        torch.cuda.synchronize()
        e.infer_device(comp, qp, p[0], p[1], p[2], n, qt.data_ptr(), bt.data_ptr(), dire.data_ptr())
        e.synchronize()
        return qt.cpu().numpy(), bt.cpu().numpy(), dire.cpu().numpy(), None
    q = torch.from_numpy(np.ascontiguousarray(qt_in, np.float32)).cuda()
    torch.cuda.synchronize()
    e.infer_msbd_device(comp, qp, p[0], p[1], p[2], q.data_ptr(), n, bt.data_ptr(), dire.data_ptr())
    e.synchronize()
    return None, bt.cpu().numpy(), dire.cpu().numpy(), q.cpu().numpy()


@pytest.mark.parametrize("comp", ["Luma", "Chroma"])
def test_infer_msbd_with_the_qt_nets_logits_is_infer_bit_for_bit(comp):
    from pmp_vvc_tip2023_amd import engine, synth
    n = 1100                                      # overlap mode cuts calls of >= 1024 blocks
    y, u, v = synth.recipe_r_blocks(n, 321)
    e = engine.Engine(0, allow_synthetic_mtt=True)
    try:
        e.load(comp, 27)
        for prec in ("f16x3", "bf16x6", "fp32"):
            e.set_precision(prec)
            for fusion, overlap, m in ((1, 0, 150), (0, 0, 150), (1, 1, n)):
                e.set_fusion(fusion); e.set_overlap(overlap)
                qt, bt, dire, _ = _infer_dev(e, comp, 27, y[:m], u[:m], v[:m])
                _, bt2, dire2, q_after = _infer_dev(e, comp, 27, y[:m], u[:m], v[:m], qt_in=qt)
                assert bt2.tobytes() == bt.tobytes() and dire2.tobytes() == dire.tobytes(), (prec, fusion, overlap)
                assert q_after.tobytes() == qt.tobytes()                     # qt_in is never written
            e.set_fusion(1); e.set_overlap(0)
        # the host-pointer form, chunked
        e.set_precision("f16x3")
        qt, bt, dire = e.inference_pre_QBD(comp, 27, y[:40], u[:40], v[:40])
        e.set_chunk(16)
        bt2, dire2 = e.infer_msbd(comp, 27, qt, y[:40], u[:40], v[:40])
        assert bt2.tobytes() == bt.tobytes() and dire2.tobytes() == dire.tobytes()
        assert e.saturation_reruns() == 0
    finally:
        e.close()


def test_infer_msbd_with_label_maps_vs_oracle():
    """Label-valued qt_in (float(qt8 - 1), 255.0 for raw 0 included) on the trained-like MTT weights: within 1e-3 of the oracle's MTT net."""
    import torch as T
    import trained_like as TL
    from oracle import nets_torch as O
    from pmp_vvc_tip2023_amd import engine, synth, weights as W
    n = 48
    y, _, _ = synth.recipe_r_blocks(n, 555)
    qt8, _, _ = K.labels(n, 556)
    qt_in = (qt8 - np.uint8(1)).astype(np.float32).reshape(n, 1, 8, 8)
    assert qt_in.max() == 255.0
    wq, _ = W.load_net_weights("Luma_Q", 22)
    wb = TL.msbd_weights("Luma", 22)
    x = O.luma_input(y)
    with T.no_grad():
        o = O.msbd_forward(wb, x, T.from_numpy(qt_in), True)
    obt = T.cat([t[:, 0:1] for t in o], 1).numpy()
    odire = T.cat([t[:, 1:2] for t in o], 1).numpy()
    e = engine.Engine(0)
    try:
        e.load("Luma", 22, q_weights=wq, msbd_weights=wb)
        for prec in ("f16x3", "bf16x6", "fp32"):
            e.set_precision(prec)
            bt, dire = e.infer_msbd("Luma", 22, qt_in, y)
            err = max(np.abs(bt - obt).max(), np.abs(dire - odire).max())
            print("teacher-forced %s: max |logit - oracle| = %.3g" % (prec, err))
            assert err < TOL, (prec, err)
    finally:
        e.close()


# ---- 5. statistics enqueued behind a call that the range guard re-runs
def test_stats_behind_a_rerun_are_those_of_the_final_logits():
    import torch
    from oracle import range_cases as R
    from pmp_vvc_tip2023_amd import engine
    cases, _, (wq, wb), _ = R.cases_for("Luma")
    case = next(c for c in cases if c.net == "bd" and c.preserving)
    gq, gb = case.apply(wq, wb, case.s_over)
    y, _, _ = R.gpu_blocks()
    n = len(y)
    qt8, msbt, msdire = K.labels(n, 77)
    e = engine.Engine(0)
    try:
        e.set_precision("f16x3")
        e.set_activation_scales(False)            # exponents of zero: the gained tensor leaves the fp16 range
        e.load("Luma", 22, q_weights=gq, msbd_weights=gb)
        d_y = torch.from_numpy(np.ascontiguousarray(y)).cuda()
        lab = [torch.from_numpy(a).cuda() for a in (qt8, msbt, msdire)]
        qt = torch.zeros((n, 64), device="cuda"); bt = torch.zeros((n, 768), device="cuda"); dire = torch.zeros((n, 768), device="cuda")
        S = torch.zeros((3, 20), dtype=torch.float64, device="cuda")
        B = torch.zeros((n, 20), dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()

        def stats(row, blk=None):
            e.val_stats_device(22, qt.data_ptr(), bt.data_ptr(), dire.data_ptr(), *[t.data_ptr() for t in lab], n,
                               S.data_ptr() + row * 160, blk)
        r0 = e.saturation_reruns()
        e.infer_device("Luma", 22, d_y.data_ptr(), None, None, n, qt.data_ptr(), bt.data_ptr(), dire.data_ptr())
        stats(0, B.data_ptr())
        e.synchronize()
        assert e.saturation_reruns() == r0 + 1
        stats(1)                                  # a second call made after the synchronize: the same bits
        e.synchronize()
        s = S.cpu().numpy()
        assert s[0].tobytes() == s[1].tobytes()
        want = K.block_stats(22, qt=qt.cpu().numpy().reshape(n, 8, 8), bt=bt.cpu().numpy().reshape(n, 3, 16, 16),
                             dire=dire.cpu().numpy().reshape(n, 3, 16, 16), qt8=qt8, msbt=msbt, msdire=msdire)
        same(B.cpu().numpy(), want, "replayed per-block")
        same(s[0], want.sum(axis=0), "replayed")
        # the same for the teacher-forced call: its re-run repeats the MTT net only
        q_in = qt.clone()
        bt.zero_(); dire.zero_()
        torch.cuda.synchronize()
        e.infer_msbd_device("Luma", 22, d_y.data_ptr(), None, None, q_in.data_ptr(), n, bt.data_ptr(), dire.data_ptr())
        stats(2)
        e.synchronize()
        assert e.saturation_reruns() == r0 + 2
        s = S.cpu().numpy()
        assert s[2].tobytes() == s[0].tobytes()   # qt_in = the QT logits: the logits of the first call, so its statistics
        assert q_in.cpu().numpy().tobytes() == qt.cpu().numpy().tobytes()
    finally:
        e.close()


# ---- 6. real nets end to end
_DATAPATH_HITS = {}


@pytest.mark.parametrize("comp,qp", [("Luma", 22), ("Chroma", 32)])
def test_real_nets_stats_vs_restatement_and_oracle(eng, comp, qp):
    # the 512 blocks of tests/test_gpu_parity.py: their oracle is computed once for both files
    y, u, v, oq, obt, odire = Y.fresh_oracle(comp, qp, 512, 1000 + qp + (7 if comp == "Chroma" else 0))
    n = len(y)
    qt8, msbt, msdire = K.labels(n, 4000 + qp)
    lab = dict(qt8=qt8, msbt=msbt, msdire=msdire)
    ref = K.stats(qp, qt=oq.reshape(n, 8, 8), bt=obt, dire=odire, **lab)
    # cells whose oracle logit lies within the logit tolerance of a rounding boundary may round the other way
    near = lambda a: (np.abs(a - np.floor(a) - 0.5) <= TOL).reshape(n, -1)
    slack = np.array([near(oq).sum()] + [near(obt[:, k]).sum() for k in range(3)] + [near(odire[:, k]).sum() for k in range(3)], np.float64)
    hits = {}
    for prec in ("f16x3", "bf16x6", "fp32"):
        eng.set_precision(prec)
        try:
            qt, bt, dire = eng.inference_pre_QBD(comp, qp, y, u, v)
            got = eng.val_stats(qp, qt=qt, bt=bt, dire=dire, **lab)
        finally:
            eng.set_precision("f16x3")
        assert Y.per_block_error((qt, bt, dire), (oq, obt, odire)).max() < TOL
        same(got, K.stats(qp, qt=qt.reshape(n, 8, 8), bt=bt, dire=dire, **lab), prec)          # on the device's own logits
        hits[prec] = got[K.COUNTS]
        print("%s QP%d %s: hits %s, oracle %s, near-boundary cells %s" % (comp, qp, prec, got[K.COUNTS].astype(int), ref[K.COUNTS].astype(int),
                                                                       slack.astype(int)))
        assert np.all(np.abs(got[K.COUNTS] - ref[K.COUNTS]) <= slack), (prec, got[K.COUNTS] - ref[K.COUNTS], slack)
    for a in hits:
        for b in hits:
            assert np.all(np.abs(hits[a] - hits[b]) <= slack), (a, b)
    # the engine's validation on the real nets = the statistics of the logits the nets return, batch by batch
    res = eng.validation_QBD(comp, qp, (y, u, v) if comp == "Chroma" else y, qt8, msbt, msdire, batch_size=200)
    qt, bt, dire = eng.inference_pre_QBD(comp, qp, y, u, v)
    c = dict(qp=qp, n=n, batch=200, qt=qt.reshape(n, 8, 8), bt=bt, dire=dire, **lab)
    mine, _ = K.numbers(*K.case_stats(c), "qbd")
    assert K.rel_dist(np.array(res), mine) <= SUM_TOL and np.array_equal(np.array(res)[K.EXACT["qbd"]], mine[K.EXACT["qbd"]])
    # pre_validation 1 = teacher-forced
    res1 = eng.pre_validation(comp, qp, 1, (y, u, v) if comp == "Chroma" else y, qt8, msbt, msdire, batch_size=200)
    bt1, dire1 = eng.infer_msbd(comp, qp, (qt8 - np.uint8(1)).astype(np.float32), y, u, v)
    c1 = dict(c, bt=bt1, dire=dire1)
    mine1, _ = K.numbers(*K.case_stats(c1, "bd"), "bd")
    assert K.rel_dist(np.array(res1), mine1) <= SUM_TOL and np.array_equal(np.array(res1)[K.EXACT["bd"]], mine1[K.EXACT["bd"]])
    res0 = eng.pre_validation(comp, qp, 0, (y, u, v) if comp == "Chroma" else y, qt8, batch_size=200)
    mine0, _ = K.numbers(*K.case_stats(c, "q"), "q")
    assert K.rel_dist(np.array(res0), mine0) <= SUM_TOL and res0[1] == mine0[1]


# ---- 7. the CLI
def test_cli_equals_engine(eng, tmp_path, capsys):
    from pmp_vvc_tip2023_amd import synth, validate
    n, qp = 230, 27
    y, u, v = synth.recipe_r_blocks(n, 808)
    qt8, msbt, msdire = K.labels(n, 809)
    d = str(tmp_path)
    np.save(os.path.join(d, "Validate_Y_Block68.npy"), y)
    np.save(os.path.join(d, "Validate_U_Block34.npy"), u)
    np.save(os.path.join(d, "Validate_V_Block34.npy"), v)
    for comp in ("Luma", "Chroma"):
        stem = os.path.join(d, "Validate_%s_QP%d_" % (comp, qp))
        np.save(stem + "QTdepth_Block8.npy", qt8)
        np.save(stem + "MSBTdepth_Block16.npy", msbt)
        np.save(stem + "MSdirection_Block16.npy", msdire)
    for comp, mode in (("Luma", "qbd"), ("Chroma", "qbd"), ("Luma", "bd"), ("Luma", "q")):
        per = os.path.join(d, "per_%s_%s.npy" % (comp, mode))
        capsys.readouterr()
        rc = validate.main(["--dataDir", d, "--comp", comp, "--qp", str(qp), "--mode", mode, "--batchSize", "100", "--perBlock", per,
                            "--allowSyntheticMtt"])
        assert rc == 0
        out = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
        blocks = (y, u, v) if comp == "Chroma" else y
        if mode == "qbd":
            want, blk = eng.validation_QBD(comp, qp, blocks, qt8, msbt, msdire, batch_size=100, return_block_stats=True)
        else:
            want, blk = eng.pre_validation(comp, qp, 0 if mode == "q" else 1, blocks, qt8, msbt, msdire, batch_size=100, return_block_stats=True)
        assert [out[k] for k in validate.NAMES[mode]] == want
        assert (out["blocks"], out["batches"], out["batch_size"], out["comp"], out["mode"]) == (n, 3, 100, comp, mode)
        pb = np.load(per)
        assert pb.shape == (n, 20) and pb.dtype == np.float64 and pb.tobytes() == blk.tobytes()
        S = np.stack([pb[o:o + 100].sum(axis=0) for o in range(0, n, 100)])
        from pmp_vvc_tip2023_amd import engine
        assert K.rel_dist(np.array(engine.validation_numbers(S, [100, 100, 30], mode)), np.array(want)) <= SUM_TOL
