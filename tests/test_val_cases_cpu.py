"""CPU: the numpy restatement of the validation statistics (tests/val_cases.py) against the reference-made G12
(tests/golden/g12_val.npz; tools/gen_golden_val.py) and against the live reference where its checkout is present; the engine's
result lists from statistics; the validate CLI's flag and shape checks, which must exit 2 before anything touches a GPU."""
import os

import numpy as np
import pytest

from conftest import golden
import ref_harness
import val_cases as K

MODES = (("qbd", "vqbd", "loss_qbd"), ("q", "pre0", None), ("bd", "pre1", "loss_msbd"))


@pytest.fixture(scope="module")
def g12():
    return golden("g12_val.npz")


@pytest.mark.parametrize("name", list(K.CASES))
def test_restatement_equals_reference_golden(g12, name):
    c = K.make(name)
    tol = float(g12["ref_vs_f64"])
    assert 0 < tol < 1e-5
    for mode, key, lkey in MODES:
        S, ns = K.case_stats(c, mode)
        mine, loss = K.numbers(S, ns, mode)
        ref = g12["%s_%s" % (name, key)]
        ex = K.EXACT[mode]
        assert np.array_equal(mine[ex], ref[ex]), (name, mode)                 # accuracies: ratios of integers
        d = K.rel_dist(ref, mine)
        print("%s %s: restatement vs reference %.3g (recorded %.3g)" % (name, mode, d, tol))
        assert d <= tol, (name, mode, d)
        if lkey:
            assert K.rel_dist(g12["%s_%s" % (name, lkey)], loss) <= tol


def test_cases_hold_what_they_promise():
    c = K.make("qp22")
    assert (c["qt8"] == 0).any() and K.loader_labels(c["qt8"], c["msbt"], c["msdire"])[0].max() == 255.0     # the u8 wrap
    for a in (c["qt"], c["bt"], c["dire"]):
        fr = a - np.floor(a)
        halves = a[fr == 0.5]
        assert (np.floor(halves) % 2 == 0).any() and (np.floor(halves) % 2 == 1).any()                      # both parities
        assert (a == np.float32(0.5)).any() and (a == np.float32(-0.5)).any()
        assert (a == np.nextafter(np.float32(2.5), np.float32(3))).any() and (a == np.nextafter(np.float32(2.5), np.float32(2))).any()
    assert all(n % b for _, n, b, _, _ in K.CASES.values())                                                   # ragged tails
    assert sorted({q for q, *_ in K.CASES.values()}) == [22, 27, 32, 37, 41]
    nf = K.make("nonfinite")
    assert np.isnan(nf["qt"]).any() and np.isposinf(nf["bt"]).any() and np.isneginf(nf["dire"]).any()
    S, _ = K.case_stats(nf)
    assert np.isnan(S[0, 0]) and np.isinf(S[0, 1]) and np.isfinite(S[1]).all() and np.isfinite(S[:, K.COUNTS]).all()
    # half to even, and the wrap, on a hand-made block
    qt = np.zeros((1, 8, 8), np.float32); qt8 = np.ones((1, 8, 8), np.uint8)
    qt[0, 0, :4] = [0.5, 1.5, 2.5, -0.5]; qt8[0, 0, :4] = [1, 3, 3, 1]
    qt[0, 1, 0] = 255.0; qt8[0, 1, 0] = 0
    s = K.stats(22, qt=qt, qt8=qt8)
    assert s[13] == 64 and s[0] == 0.5 + 0.5 + 0.5 + 0.5


def test_engine_result_lists_equal_the_restatement():
    from pmp_vvc_tip2023_amd import engine
    c = K.make("qp32")
    for mode, _, _ in MODES:
        S, ns = K.case_stats(c, mode)
        mine, _ = K.numbers(S, ns, mode)
        got = np.array(engine.validation_numbers(S, ns, mode))
        assert got.shape == mine.shape and K.rel_dist(got, mine) <= 1e-15
    assert np.array_equal(engine.VAL_ELEMS, K.ELEMS)


def test_runs_of_batch_ranges_join_into_the_whole_run_and_the_mode_tables():
    """ValRun.join over every split point of a case's batches, an empty share at either end included: the whole run's numbers as bytes
    and its confusion counts, for all three modes; the per-mode tables against the literals the CLI printed from its own copies."""
    import confusion_cases as X
    from pmp_vvc_tip2023_amd import validation as V
    c = K.make("qp41_small")
    per_block = X.block_counts(**{k: c[k] for k in X.ORDER})
    conf = np.stack([per_block[o:o + m].sum(axis=0) for o, m in K.batches(c)])
    names = {"qbd": ["q_L1", "b0_L1", "b1_L1", "b2_L1", "d0_L1", "d1_L1", "d2_L1", "q_accu", "b0_accu", "b1_accu", "b2_accu", "d0_accu",
                     "d1_accu", "d2_accu", "val_loss"],
             "q": ["q_L1", "q_accu"],
             "bd": ["b0_L1", "b1_L1", "b2_L1", "d0_L1", "d1_L1", "d2_L1", "b0_accu", "b1_accu", "b2_accu", "d0_accu", "d1_accu", "d2_accu",
                    "val_loss"]}
    maps = {"q": ("qt",), "bd": ("bt0", "bt1", "bt2", "dire0", "dire1", "dire2"), "qbd": ("qt", "bt0", "bt1", "bt2", "dire0", "dire1", "dire2")}
    assert V.MODES == ("qbd", "q", "bd") and [V.mode_of_pred(p) for p in (0, 1, 2)] == ["q", "bd", "qbd"]
    for mode, count in zip(V.MODES, (15, 2, 13)):
        S, ns = K.case_stats(c, mode)
        assert len(ns) == 3
        whole = V.ValRun(mode, S, ns, None, conf)
        want = np.array(whole.numbers())
        assert want.tobytes() == np.array(V.validation_numbers(S, ns, mode)).tobytes() and K.rel_dist(want, K.numbers(S, ns, mode)[0]) <= 1e-15
        assert np.array_equal(whole.confusion(), per_block.sum(axis=0))
        for cut in range(len(ns) + 1):
            j = V.ValRun.join([V.ValRun(mode, S[:cut], ns[:cut], None, conf[:cut]), V.ValRun(mode, S[cut:], ns[cut:], None, conf[cut:])])
            assert j.mode == mode and j.ns == ns and j.S.tobytes() == S.tobytes() and j.conf.tobytes() == conf.tobytes()
            assert np.array(j.numbers()).tobytes() == want.tobytes()
            assert np.array_equal(j.confusion(), whole.confusion())
        singles = V.ValRun.join(V.ValRun(mode, S[i:i + 1], ns[i:i + 1]) for i in range(len(ns)))
        assert np.array(singles.numbers()).tobytes() == want.tobytes() and singles.conf is None
        assert V.NAMES[mode] == names[mode] and len(V.NAMES[mode]) == len(want) == count
        assert tuple(V.CONF_MAPS[i] for i in V.MODE_MAPS[mode]) == maps[mode]


@pytest.mark.skipif(not ref_harness.available(), reason="reference checkout not present")
def test_restatement_equals_live_reference(g12):
    import torch
    _, Metrics, _, _ = ref_harness.load()
    c = K.make("qp41_small")
    qt = torch.from_numpy(c["qt"]).reshape(-1, 1, 8, 8)
    bt, dire = torch.from_numpy(c["bt"]), torch.from_numpy(c["dire"])
    ql = torch.FloatTensor(np.expand_dims(c["qt8"], 1) - 1)
    assert float(ql.max()) == 255.0                                            # the loader's expression wraps
    bl, dl = torch.FloatTensor(c["msbt"]), torch.FloatTensor(c["msdire"])
    ld = [(torch.arange(o, o + m), ql[o:o + m], bl[o:o + m], dl[o:o + m]) for o, m in K.batches(c)]
    ref = np.array(Metrics.validation_QBD(ld, lambda i: qt[i], lambda i, q: tuple(torch.stack([bt[i, k], dire[i, k]], 1) for k in range(3)),
                                          c["qp"]), np.float64)
    assert np.array_equal(ref, g12["qp41_small_vqbd"], equal_nan=True)
    mine, _ = K.numbers(*K.case_stats(c), "qbd")
    assert np.array_equal(mine[K.EXACT["qbd"]], ref[K.EXACT["qbd"]]) and K.rel_dist(ref, mine) <= float(g12["ref_vs_f64"])


def _write_set(d, n=6, comp="Luma", qp=27, data_type="Validate"):
    c = K.make("qp27")
    np.save(os.path.join(d, "%s_Y_Block68.npy" % data_type), np.zeros((n, 68, 68), np.uint8))
    if comp == "Chroma":
        np.save(os.path.join(d, "%s_U_Block34.npy" % data_type), np.zeros((n, 34, 34), np.uint8))
        np.save(os.path.join(d, "%s_V_Block34.npy" % data_type), np.zeros((n, 34, 34), np.uint8))
    stem = os.path.join(d, "%s_%s_QP%d_" % (data_type, comp, qp))
    np.save(stem + "QTdepth_Block8.npy", c["qt8"][:n])
    np.save(stem + "MSBTdepth_Block16.npy", c["msbt"][:n])
    np.save(stem + "MSdirection_Block16.npy", c["msdire"][:n])
    return stem


def test_cli_refuses_bad_flags_and_shapes_before_the_gpu(tmp_path, monkeypatch, capsys):
    from pmp_vvc_tip2023_amd import engine, validate

    def no_engine(*a, **k):
        raise AssertionError("the CLI created an Engine before its checks were done")
    monkeypatch.setattr(engine, "Engine", no_engine)
    d = str(tmp_path)
    stem = _write_set(d)
    good = ["--dataDir", d, "--comp", "Luma", "--qp", "27"]
    plan = validate.plan(validate.build_parser().parse_args(good))
    assert plan["n"] == 6 and plan["msbt"].shape == (6, 3, 16, 16)

    def rc(argv):
        with pytest.raises(SystemExit) as ei:
            validate.main(argv)
        return ei.value.code
    assert rc(["--dataDir", d, "--comp", "Lumma", "--qp", "27"]) == 2
    assert rc(["--dataDir", d, "--comp", "Luma", "--qp", "21"]) == 2
    assert rc(["--dataDir", d, "--comp", "Luma", "--qp", "42"]) == 2
    assert rc(good + ["--mode", "d"]) == 2
    assert rc(good + ["--batchSize", "0"]) == 2
    assert rc(good + ["--precision", "fp16"]) == 2
    assert rc(good + ["--dataType", "Train"]) == 2                            # no such files
    assert rc(good + ["--modelDir", os.path.join(d, "nope")]) == 2
    assert rc(good + ["--perBlock", os.path.join(d, "nope", "b.npy")]) == 2
    assert rc(["--dataDir", os.path.join(d, "nope"), "--comp", "Luma", "--qp", "27"]) == 2
    assert rc(["--dataDir", d, "--comp", "Chroma", "--qp", "27"]) == 2       # no chroma files
    np.save(stem + "MSdirection_Block16.npy", np.zeros((6, 3, 16, 16), np.uint8))          # wrong dtype
    assert rc(good) == 2
    assert "int8" in capsys.readouterr().err
    np.save(stem + "MSdirection_Block16.npy", np.zeros((5, 3, 16, 16), np.int8))           # wrong count
    assert rc(good) == 2
    assert validate.plan(validate.build_parser().parse_args(good + ["--mode", "q"]))["n"] == 6      # mode q does not read it
    np.save(stem + "QTdepth_Block8.npy", np.zeros((6, 64), np.uint8))                      # wrong shape
    assert rc(good + ["--mode", "q"]) == 2
