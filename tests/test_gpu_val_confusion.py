"""GPU: confusion counts (include/pmp.h: pmp_val_confusion, logitstats.hip), the QT-only inference call (pmp_infer_q) and what the
engine, validate and train_qbd make of them.

Nothing here has a tolerance.  Counts are integers and compared exactly with the numpy restatement (tests/confusion_cases.py, pinned on
the CPU by test_confusion_cases_cpu.py); pmp_infer_q's logits are compared with pmp_infer's bit for bit; files byte for byte."""
import json
import os
import signal
import subprocess
import sys

import numpy as np
import pytest

import confusion_cases as X
import gpu_rig
import train_qbd_cases as TC
import val_cases as K
from conftest import ROOT

pytestmark = pytest.mark.gpu

eng = gpu_rig.engine_fixture(synthetic_mtt=True)
POISON16, POISON64 = 0x5A5A, -0x0123456789ABCDEF


def dev_counts(e, kw, block_counts=False, sync=True):
    """pmp_val_confusion_device on uploaded copies, outputs poisoned before the call -> (int64[7,5,5], per-block u16[n,175] or None)"""
    import torch
    d = {k: torch.from_numpy(np.ascontiguousarray(kw[k])).cuda() if k in kw else None for k in X.ORDER}
    n = len(kw["qt8"] if "qt8" in kw else kw["msbt"])
    C = torch.full((X.NCOUNTS,), POISON64, dtype=torch.int64, device="cuda")
    B = torch.full((n, X.NCOUNTS), POISON16, dtype=torch.int16, device="cuda") if block_counts else None
    torch.cuda.synchronize()
    e.val_confusion_device(*[None if d[k] is None else d[k].data_ptr() for k in X.ORDER], n, C.data_ptr(), None if B is None else B.data_ptr())
    e.synchronize()
    torch.cuda.synchronize()
    return C.cpu().numpy().reshape(7, 5, 5), (None if B is None else B.cpu().numpy().view(np.uint16))


@pytest.fixture(scope="module")
def case200():
    c = X.in_range(200, 11)
    return c, X.block_counts(**c)


# ---- 1. the device form against the restatement
@pytest.mark.parametrize("n", [1, 3, 17, 200])
def test_device_counts_equal_the_restatement_in_every_form(eng, case200, n):
    c, blocks = case200
    s = slice(0, n)
    for name in X.FORMS:
        kw = X.form(c, name, s)
        want = X.block_counts(**kw) if name != "both" else blocks[s]
        got, _ = dev_counts(eng, kw)
        assert np.array_equal(got, want.sum(axis=0)), (name, n)
        got2, blk = dev_counts(eng, kw, block_counts=True)
        assert got2.tobytes() == got.tobytes(), (name, n)
        assert np.array_equal(blk.astype(np.int64).reshape(n, 7, 5, 5), want), (name, n)     # every element written: no poison left
        assert np.array_equal(blk.astype(np.int64).sum(axis=0).reshape(7, 5, 5), got), (name, n)
    full = blocks[s].sum(axis=0)
    cen, _ = dev_counts(eng, X.form(c, "census", s))
    assert np.array_equal(cen.sum(axis=2), full.sum(axis=2))        # the census' row sums are the label counts
    assert not cen[:4, :, :4].any() and not cen[4:, :, :3].any() and not cen[4:, :, 4].any()


def test_special_values(eng):
    c = X.special(2)
    want = X.block_counts(**c)
    got, blk = dev_counts(eng, c, block_counts=True)
    assert np.array_equal(blk.astype(np.int64).reshape(2, 7, 5, 5), want)
    assert np.array_equal(got, want.sum(axis=0))
    assert got[0, 4].sum() >= 32 and got[1, 4].sum() >= 32 and got[4, 3].sum() >= 48      # the "other" labels are really there
    # one cell per block: every special logit against a plain label, on each kind of map
    for x, d, r in X.SPECIAL_LOGITS:
        one = dict(qt=np.full((1, 8, 8), x, np.float32), qt8=np.full((1, 8, 8), 2, np.uint8), bt=np.full((1, 3, 16, 16), x, np.float32),
                   dire=np.full((1, 3, 16, 16), x, np.float32), msbt=np.zeros((1, 3, 16, 16), np.uint8), msdire=np.ones((1, 3, 16, 16), np.int8))
        got, _ = dev_counts(eng, one)
        assert got[0, 1, d] == 64 and all(got[1 + k, 0, d] == 256 for k in range(3)) and all(got[4 + k, 2, r] == 256 for k in range(3)), x


# ---- 2. the tie to the reference's accuracy
def test_diagonal_equals_val_stats_hit_counts(eng, case200):
    import torch
    c, blocks = case200
    d = {k: torch.from_numpy(c[k]).cuda() for k in X.ORDER}
    S = torch.zeros(20, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    eng.val_stats_device(27, *[d[k].data_ptr() for k in X.ORDER], 200, S.data_ptr())
    eng.synchronize()
    got, _ = dev_counts(eng, c)
    assert X.diagonal(got).tolist() == S.cpu().numpy()[13:20].astype(np.int64).tolist()
    assert X.diagonal(got).tolist() == K.stats(27, **c)[13:20].astype(np.int64).tolist()


# ---- 3. the host form, n = 0 and the invalid calls
def test_host_form_chunks_empty_and_invalid_calls(eng, case200):
    import torch
    from pmp_vvc_tip2023_amd import _lib
    c, blocks = case200
    s = slice(0, 5)
    dev, _ = dev_counts(eng, X.form(c, "both", s))
    eng.set_chunk(2)                                  # 5 blocks = 3 passes, whose counts are added
    try:
        for name in X.FORMS:
            host = eng.val_confusion(**X.form(c, name, s))
            assert host.dtype == np.int64 and np.array_equal(host, X.counts(**X.form(c, name, s))), name
            if name == "both":
                assert host.tobytes() == dev.tobytes()
    finally:
        eng.set_chunk(4096)
    z = eng.val_confusion(**X.form(c, "both", slice(0, 0)))
    assert z.shape == (7, 5, 5) and not z.any()
    C = torch.full((X.NCOUNTS,), 7, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    eng.val_confusion_device(None, None, None, None, None, None, 0, C.data_ptr())
    eng.synchronize()
    assert not C.cpu().numpy().any()

    # every invalid form: PMP_E_INVALID, nothing written
    n = 4
    d = {k: torch.from_numpy(np.ascontiguousarray(c[k][:n])).cuda() for k in X.ORDER}
    C = torch.full((X.NCOUNTS + 1,), POISON64, dtype=torch.int64, device="cuda")
    B = torch.full((n * X.NCOUNTS + 1,), POISON16, dtype=torch.int16, device="cuda")
    torch.cuda.synchronize()
    p = {k: t.data_ptr() for k, t in d.items()}

    def call(count=n, counts=C.data_ptr(), blk=B.data_ptr(), **over):
        a = dict(p, **over)
        return eng.lib.pmp_val_confusion_device(eng.h, a["qt"], a["bt"], a["dire"], a["qt8"], a["msbt"], a["msdire"], count, counts, blk)
    bad = {"qt without qt8": dict(qt8=None), "bt, dire without their labels": dict(msbt=None, msdire=None), "bt without dire": dict(dire=None),
           "dire without bt": dict(bt=None), "msbt without msdire": dict(msdire=None, bt=None, dire=None),
           "msdire without msbt": dict(msbt=None, bt=None, dire=None), "no labels at all": dict(qt=None, bt=None, dire=None, qt8=None, msbt=None, msdire=None),
           "logits only": dict(qt8=None, msbt=None, msdire=None), "bt misaligned": dict(bt=p["bt"] + 4), "dire misaligned": dict(dire=p["dire"] + 8),
           "qt misaligned": dict(qt=p["qt"] + 2), "msbt misaligned": dict(msbt=p["msbt"] + 1), "msdire misaligned": dict(msdire=p["msdire"] + 2)}
    for what, over in bad.items():
        assert call(**over) == -1, what
    assert call(count=-1) == -1 and call(counts=None) == -1
    assert call(counts=C.data_ptr() + 4) == -1 and call(blk=B.data_ptr() + 1) == -1
    eng.synchronize()
    torch.cuda.synchronize()
    assert (C.cpu().numpy() == POISON64).all() and (B.cpu().numpy() == POISON16).all()
    assert call() == 0                                # the rig itself is sound: the same call without a fault passes ...
    assert call(counts=C.data_ptr() + 8, blk=B.data_ptr() + 2) == 0                # ... at the smallest alignments too
    eng.synchronize()
    want = X.counts(**X.form(c, "both", slice(0, n)))
    assert np.array_equal(C.cpu().numpy()[1:].reshape(7, 5, 5), want)
    # the host form's checks
    out = np.full(X.NCOUNTS, 3, np.int64)
    h = {k: np.ascontiguousarray(c[k][:n]) for k in X.ORDER}
    P = lambda a: None if a is None else a.ctypes.data
    for over in (dict(qt8=None), dict(dire=None), dict(msdire=None, bt=None, dire=None), dict(qt=None, bt=None, dire=None, qt8=None, msbt=None, msdire=None)):
        a = dict(h, **over)
        assert eng.lib.pmp_val_confusion(eng.h, *[P(a[k]) for k in X.ORDER], n, P(out)) == -1
    assert eng.lib.pmp_val_confusion(eng.h, *[P(h[k]) for k in X.ORDER], -1, P(out)) == -1
    assert eng.lib.pmp_val_confusion(eng.h, *[P(h[k]) for k in X.ORDER], n, None) == -1
    assert (out == 3).all()
    with pytest.raises(ValueError):
        eng.val_confusion(qt=h["qt"])
    assert isinstance(_lib.PMP_CONF_NCOUNTS, int)


# ---- 4. a confusion call behind an inference call that the range guard re-runs
def test_counts_behind_a_rerun_are_those_of_the_final_logits():
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
        C = torch.full((2, X.NCOUNTS), POISON64, dtype=torch.int64, device="cuda")
        B = torch.full((n, X.NCOUNTS), POISON16, dtype=torch.int16, device="cuda")
        torch.cuda.synchronize()

        def conf(row, blk=None):
            e.val_confusion_device(qt.data_ptr(), bt.data_ptr(), dire.data_ptr(), *[t.data_ptr() for t in lab], n, C.data_ptr() + row * X.NCOUNTS * 8, blk)
        r0 = e.saturation_reruns()
        e.infer_device("Luma", 22, d_y.data_ptr(), None, None, n, qt.data_ptr(), bt.data_ptr(), dire.data_ptr())
        conf(0, B.data_ptr())
        e.synchronize()
        assert e.saturation_reruns() == r0 + 1
        conf(1)                                   # a second call made after the synchronize: the same bytes
        e.synchronize()
        c = C.cpu().numpy()
        assert c[0].tobytes() == c[1].tobytes()
        want = X.block_counts(qt=qt.cpu().numpy().reshape(n, 8, 8), bt=bt.cpu().numpy().reshape(n, 3, 16, 16),
                              dire=dire.cpu().numpy().reshape(n, 3, 16, 16), qt8=qt8, msbt=msbt, msdire=msdire)
        assert np.array_equal(B.cpu().numpy().view(np.uint16).astype(np.int64).reshape(n, 7, 5, 5), want)
        assert np.array_equal(c[0].reshape(7, 5, 5), want.sum(axis=0))
    finally:
        e.close()


# ---- 5. pmp_infer_q
def _infer_both(e, comp, qp, y, u, v):
    """pmp_infer_device and pmp_infer_q_device on the same blocks -> (qt of infer, qt of infer_q)"""
    import torch
    n = len(y)
    d = [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in ((y, u, v) if comp == "Chroma" else (y,))]
    p = [t.data_ptr() for t in d] + [None] * (3 - len(d))
    qt = torch.zeros((n, 64), device="cuda"); bt = torch.zeros((n, 768), device="cuda"); dire = torch.zeros((n, 768), device="cuda")
    q2 = torch.full((n, 64), float("nan"), device="cuda")
    torch.cuda.synchronize()
    e.infer_device(comp, qp, p[0], p[1], p[2], n, qt.data_ptr(), bt.data_ptr(), dire.data_ptr())
    e.infer_q_device(comp, qp, p[0], p[1], p[2], n, q2.data_ptr())
    e.synchronize()
    return qt.cpu().numpy(), q2.cpu().numpy()


@pytest.mark.parametrize("comp", ["Luma", "Chroma"])
def test_infer_q_is_infers_qt_bit_for_bit(eng, comp):
    from pmp_vvc_tip2023_amd import synth
    y, u, v = synth.recipe_r_blocks(5, 4321)
    eng.load(comp, 27)
    try:
        for prec in gpu_rig.DATAPATHS:
            eng.set_precision(prec)
            for chunk, overlap in ((4096, 0), (2, 0), (2, 1)):
                eng.set_chunk(chunk); eng.set_overlap(overlap)
                a, b = _infer_both(eng, comp, 27, y, u, v)
                assert a.tobytes() == b.tobytes(), (prec, chunk, overlap)
                host = eng.infer_q(comp, 27, y, u, v)
                assert host.shape == (5, 1, 8, 8) and host.tobytes() == a.tobytes(), (prec, chunk, overlap)
    finally:
        eng.set_precision("f16x3"); eng.set_chunk(4096); eng.set_overlap(0)
    assert eng.saturation_reruns() == 0


def test_infer_q_overlap_cut_of_a_large_call(eng):
    """Overlap mode cuts calls of at least 1024 blocks in two: the QT-only call takes the same cut"""
    from pmp_vvc_tip2023_amd import synth
    y, u, v = synth.recipe_r_blocks(1030, 99)
    eng.load("Luma", 22)
    eng.set_overlap(1)
    try:
        a, b = _infer_both(eng, "Luma", 22, y, u, v)
    finally:
        eng.set_overlap(0)
    assert a.tobytes() == b.tobytes()


def test_infer_q_needs_the_qt_net_alone(tmp_path):
    from pmp_vvc_tip2023_amd import _lib, engine, synth
    y, u, v = synth.recipe_r_blocks(5, 17)
    e = engine.Engine(0)                          # no allow_synthetic_mtt; the package's weight directory holds no *_BD_* file
    full = engine.Engine(0, allow_synthetic_mtt=True)
    try:
        with pytest.raises(FileNotFoundError):
            e.check_available("Luma", 32)
        e.check_available("Luma", 32, kinds=("Q",))
        qt = e.infer_q("Luma", 32, y)
        assert e.has_weights("Luma_Q", 32) and not e.has_weights("Luma_MSBD", 32)
        assert qt.tobytes() == full.inference_pre_QBD("Luma", 32, y)[0].tobytes()
        import torch
        t = torch.zeros(5 * (64 + 768 + 768), device="cuda")
        d_y = torch.from_numpy(y).cuda()
        torch.cuda.synchronize()
        with pytest.raises(_lib.PmpError) as ei:  # the full call still needs its MTT net
            e.infer_device("Luma", 32, d_y.data_ptr(), None, None, 5, t.data_ptr(), t.data_ptr() + 5 * 64 * 4, t.data_ptr() + 5 * (64 + 768) * 4)
        assert ei.value.code == -3
        with pytest.raises(_lib.PmpError) as ei:  # and the QT-only call its QT net
            e.infer_q_device("Luma", 37, d_y.data_ptr(), None, None, 5, t.data_ptr())
        assert ei.value.code == -3
        assert "pmp_infer_q:" in str(ei.value)     # the message names the entry point that was called
        # pre_validation 0 runs on it: same numbers as beside the synthetic MTT net, and the confusion counts of the logits
        qt8, _, _ = K.labels(5, 18)
        got, conf = e.pre_validation("Luma", 32, 0, y, qt8, batch_size=2, return_confusion=True)
        assert got == full.pre_validation("Luma", 32, 0, y, qt8, batch_size=2)
        assert not e.has_weights("Luma_MSBD", 32)
        want = X.counts(qt=qt.reshape(5, 8, 8), qt8=qt8)
        assert conf.dtype == np.int64 and np.array_equal(conf, want)
        S, ns, per = e.pre_validation("Luma", 32, 0, y, qt8, batch_size=2, return_confusion=True, batch_range=(1, 3))
        assert per.shape == (2, 7, 5, 5) and ns == [2, 1]
        assert np.array_equal(per[0], X.counts(qt=qt.reshape(5, 8, 8)[2:4], qt8=qt8[2:4])) and np.array_equal(per[1], X.counts(qt=qt.reshape(5, 8, 8)[4:], qt8=qt8[4:]))
    finally:
        e.close(); full.close()


def test_infer_q_reruns_once_on_a_q_range_case():
    import torch
    from oracle import range_cases as R
    from pmp_vvc_tip2023_amd import engine
    cases, _, (wq, wb), _ = R.cases_for("Luma")
    case = next(c for c in cases if c.net == "q" and c.preserving)
    gq, _ = case.apply(wq, wb, case.s_over)
    y, _, _ = R.gpu_blocks()
    n = len(y)
    e = engine.Engine(0)
    try:
        e.load_q("Luma", 22, q_weights=gq)
        assert not e.has_weights("Luma_MSBD", 22)
        e.set_precision("fp32")
        want = e.infer_q("Luma", 22, y)
        assert e.saturation_reruns() == 0
        e.set_precision("f16x3")
        d_y = torch.from_numpy(np.ascontiguousarray(y)).cuda()
        qt = torch.zeros((n, 64), device="cuda")
        torch.cuda.synchronize()
        e.infer_q_device("Luma", 22, d_y.data_ptr(), None, None, n, qt.data_ptr())
        e.synchronize()
        assert e.saturation_reruns() == 1 and e.saturated()
        assert qt.cpu().numpy().tobytes() == want.tobytes()
        assert e.infer_q("Luma", 22, y).tobytes() == want.tobytes() and e.saturation_reruns() == 2      # the host form too
    finally:
        e.close()


def test_engine_validation_confusion_through_batches(eng, case200):
    c, blocks = case200
    s = slice(0, 23)
    logits = (c["qt"][s], c["bt"][s], c["dire"][s])
    plain = eng.validation_QBD("Luma", 27, None, c["qt8"][s], c["msbt"][s], c["msdire"][s], batch_size=10, logits=logits)
    got, conf = eng.validation_QBD("Luma", 27, None, c["qt8"][s], c["msbt"][s], c["msdire"][s], batch_size=10, logits=logits, return_confusion=True)
    assert got == plain and np.array_equal(conf, blocks[s].sum(axis=0))
    got, blk, conf = eng.validation_QBD("Luma", 27, None, c["qt8"][s], c["msbt"][s], c["msdire"][s], batch_size=10, logits=logits,
                                        return_block_stats=True, return_confusion=True)
    assert got == plain and blk.shape == (23, 20) and np.array_equal(conf, blocks[s].sum(axis=0))
    S, ns, per = eng.validation_QBD("Luma", 27, None, c["qt8"][s], c["msbt"][s], c["msdire"][s], batch_size=10, logits=logits,
                                    return_confusion=True, batch_range=(0, 3))
    assert ns == [10, 10, 3] and np.array_equal(per, np.stack([blocks[o:o + m].sum(axis=0) for o, m in ((0, 10), (10, 10), (20, 3))]))
    got, conf = eng.pre_validation("Luma", 27, 1, None, c["qt8"][s], c["msbt"][s], c["msdire"][s], batch_size=10, logits=logits[1:], return_confusion=True)
    assert not conf[0].any() and np.array_equal(conf[1:], blocks[s].sum(axis=0)[1:])


# ---- 6. the tools
def _write_validate_set(d, comp, qp, n, seed):
    from pmp_vvc_tip2023_amd import synth
    y, u, v = synth.recipe_r_blocks(n, seed)
    qt8, msbt, msdire = K.labels(n, seed + 1)
    np.save(os.path.join(d, "Validate_Y_Block68.npy"), y)
    stem = os.path.join(d, "Validate_%s_QP%d_" % (comp, qp))
    np.save(stem + "QTdepth_Block8.npy", qt8)
    np.save(stem + "MSBTdepth_Block16.npy", msbt)
    np.save(stem + "MSdirection_Block16.npy", msdire)
    return y, qt8, msbt, msdire


def _json(capsys):
    return json.loads(capsys.readouterr().out.strip().splitlines()[-1])


def test_validate_mode_q_needs_no_bd_file_and_confusion_and_labels(eng, tmp_path, capsys):
    from pmp_vvc_tip2023_amd import engine, validate, weights as W
    qp, n = 27, 23
    d, m = str(tmp_path / "data"), str(tmp_path / "models")
    os.makedirs(d); os.makedirs(m)
    y, qt8, msbt, msdire = _write_validate_set(d, "Luma", qp, n, 808)
    W.save_pmpw(os.path.join(m, "Luma_Q_%d.pmpw" % qp), "Luma_Q", qp, W.load_net_weights("Luma_Q", qp)[0])
    base = ["--dataDir", d, "--comp", "Luma", "--qp", str(qp), "--batchSize", "10"]
    capsys.readouterr()
    assert validate.main(base + ["--mode", "q", "--modelDir", m]) == 0          # a model directory without BD files
    alone = _json(capsys)
    assert validate.main(base + ["--mode", "q", "--allowSyntheticMtt"]) == 0     # beside the synthetic MTT net, as before
    beside = _json(capsys)
    assert (alone["q_L1"], alone["q_accu"]) == (beside["q_L1"], beside["q_accu"]) and "confusion" not in alone
    want0 = eng.pre_validation("Luma", qp, 0, y, qt8, batch_size=10)
    assert [alone["q_L1"], alone["q_accu"]] == want0
    # --confusion: the summary of the counts of the logits
    assert validate.main(base + ["--mode", "q", "--modelDir", m, "--confusion"]) == 0
    out = _json(capsys)
    qt = eng.infer_q("Luma", qp, y)
    summary = engine.confusion_summary(X.counts(qt=qt.reshape(n, 8, 8), qt8=qt8))
    assert list(out["confusion"]) == ["qt"] and out["confusion"]["qt"] == json.loads(json.dumps(summary["qt"]))
    assert (out["q_L1"], out["q_accu"]) == (alone["q_L1"], alone["q_accu"])
    assert validate.main(base + ["--mode", "qbd", "--allowSyntheticMtt", "--confusion"]) == 0
    out = _json(capsys)
    qt, bt, dire = eng.inference_pre_QBD("Luma", qp, y)
    summary = engine.confusion_summary(X.counts(qt=qt.reshape(n, 8, 8), bt=bt, dire=dire, qt8=qt8, msbt=msbt, msdire=msdire))
    assert list(out["confusion"]) == list(X.NAMES) and out["confusion"] == json.loads(json.dumps(summary))
    # --mode labels: the census, with no model directory and no block file in reach
    os.remove(os.path.join(d, "Validate_Y_Block68.npy"))
    assert validate.main(["--dataDir", d, "--comp", "Luma", "--qp", str(qp), "--mode", "labels", "--modelDir", str(tmp_path / "data")]) == 0
    out = _json(capsys)
    census = engine.confusion_summary(X.counts(qt8=qt8, msbt=msbt, msdire=msdire))
    assert out["mode"] == "labels" and out["blocks"] == n and out["confusion"] == json.loads(json.dumps(census))
    assert out["confusion"]["qt"]["label_freq"] == [float(v) / (64 * n) for v in np.bincount(X.depth_class((qt8 - np.uint8(1)).astype(float)).ravel(), minlength=5)]


COMP, QP = "Chroma", 27
JOB_TIMEOUT_S = 300


@pytest.fixture(scope="module")
def sets(tmp_path_factory):
    d = tmp_path_factory.mktemp("sets")
    return d, TC.write_sets(str(d), COMP, QP)


def _files(job):
    return {k: open(os.path.join(job, k), "rb").read() for k in sorted(os.listdir(job)) if k != "last.pt"}


def test_train_qbd_pred0_confusion_file(sets, tmp_path):
    """--predID 0 --confusion, 2 epochs of 2 steps: confusion.txt holds the counts of each epoch's net on Validate and TestSub, and every
    other file is the run's without the flag.  No *_BD_* file exists anywhere the job looks."""
    import glob
    from pmp_vvc_tip2023_amd import engine, train_qbd, weights as W
    d, data = sets
    kw = dict(batchSize=5, epoch=2, saveEvery=1, maxSteps=2, seed=3)
    assert train_qbd.main(TC.argv(d, tmp_path / "plain", COMP, 0, QP, **kw)) == 0
    assert train_qbd.main(TC.argv(d, tmp_path / "conf", COMP, 0, QP, confusion=True, **kw)) == 0
    plain, conf = _files(str(tmp_path / "plain" / "0000")), _files(str(tmp_path / "conf" / "0000"))
    assert "confusion.txt" not in plain and sorted(conf) == sorted(list(plain) + ["confusion.txt"])
    for k in plain:
        assert conf[k] == plain[k], k
    want = ""
    for epoch in range(2):
        (pkl,) = glob.glob(str(tmp_path / "conf" / "0000" / ("%s_Q_%d_epoch_%d_*.pkl" % (COMP, QP, epoch))))
        e = engine.Engine(0)
        try:
            e.load_q(COMP, QP, q_weights=W.load_pkl(pkl))
            cs = []
            for name in ("Validate", "TestSub"):
                s = data[name]
                qt = e.infer_q(COMP, QP, s["y"], s["u"], s["v"])
                cs.append(X.counts(qt=qt.reshape(-1, 8, 8), qt8=s["qt8"]))
        finally:
            e.close()
        want += X.file_lines(epoch, cs, (0,))
    assert conf["confusion.txt"].decode() == want and want.count("\n") == 4
    # the .pmpw the job leaves is the last epoch's net: the job directory as model directory gives the last epoch's lines
    job = str(tmp_path / "conf" / "0000")
    assert sorted(k for k in conf if k.endswith(".pmpw")) == ["%s_Q_%d.pmpw" % (COMP, QP)]
    e = engine.Engine(0, weight_dir=job)
    try:
        cs = [X.counts(qt=e.infer_q(COMP, QP, data[name]["y"], data[name]["u"], data[name]["v"]).reshape(-1, 8, 8), qt8=data[name]["qt8"])
              for name in ("Validate", "TestSub")]
        assert e.provenance[(COMP + "_Q", QP)] == os.path.join(job, "%s_Q_%d.pmpw" % (COMP, QP))
    finally:
        e.close()
    assert X.file_lines(1, cs, (0,)) == "".join(want.splitlines(True)[2:])


def _job(d, out, **flags):
    """One run of the command in a child process of its own session, as test_gpu_train_qbd_ddp.py's -> its job directory"""
    e = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""), PMP_DIST_BACKEND="gloo", HIP_VISIBLE_DEVICES="0")
    cmd = [sys.executable, "-m", "pmp_vvc_tip2023_amd.train_qbd"] + TC.argv(d, out, COMP, 0, QP, **flags)
    p = subprocess.Popen(cmd, env=e, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, start_new_session=True)
    try:
        text, _ = p.communicate(timeout=JOB_TIMEOUT_S)
    except subprocess.TimeoutExpired:
        os.killpg(p.pid, signal.SIGKILL)
        p.communicate()
        pytest.fail("train_qbd %s did not end within %d s" % (flags, JOB_TIMEOUT_S))
    assert p.returncode == 0, "train_qbd %s ended with status %d:\n%s" % (flags, p.returncode, text[-3000:])
    return os.path.join(str(out), "0000")


def test_two_ranks_write_the_one_rank_confusion_file(sets, tmp_path):
    """Validate and TestSub have 12 blocks = 3 batches of 5, 5, 2: rank 0 runs two of them, rank 1 one; the per-batch counts travel with
    the per-batch statistics and add up to the one-rank file, byte for byte - as every other file does."""
    d, _ = sets
    kw = dict(batchSize=5, epoch=1, saveEvery=1, maxSteps=2, seed=3, confusion=True)
    one = _files(_job(d, tmp_path / "micro3", microBatch=3, **kw))
    two = _files(_job(d, tmp_path / "gpus2", gpus=2, **kw))
    assert "confusion.txt" in one and one["confusion.txt"].count(b"\n") == 2
    assert sorted(one) == sorted(two)
    for k in one:
        assert one[k] == two[k], k
