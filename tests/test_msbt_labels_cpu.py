"""CPU: the DecLib dump parser (pmp_read_depth_dump) against the reference-made G11, its refusals, the numpy restatement of GenMSBtMap
(tests/msbt_cases.py) against G11 wherever the reference finished, and gen_labels' flag and file-name handling before any GPU work."""
import os

import numpy as np
import pytest

from conftest import golden
import msbt_cases as K
from pmp_vvc_tip2023_amd import _lib, engine


@pytest.fixture(scope="module")
def lib():
    if not os.path.isfile(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.load()


@pytest.fixture(scope="module")
def g11():
    return golden("g11_msbt.npz")


@pytest.mark.parametrize("case", K.DUMPS, ids=[d[0] for d in K.DUMPS])
def test_dump_parser_matches_reference(lib, g11, tmp_path, case):
    name, seed, fw, frames, h, w, chroma, rate = case
    p = tmp_path / "d.txt"
    p.write_text(K.make_dump(seed, fw, h, w, chroma, rate))
    q, b, d, unk = engine.output_block_partition_map(str(p), w, h, frames, 64, chroma, return_unknown=True)
    assert q.dtype == np.uint8 and b.dtype == np.uint8 and d.dtype == np.int8
    assert np.array_equal(q, g11["dump_%s_qt" % name])
    assert np.array_equal(b, g11["dump_%s_bt" % name])
    assert np.array_equal(d, g11["dump_%s_dire" % name])
    assert unk == int(g11["dump_%s_unknown" % name])
    if rate:
        assert unk > 0


GOOD = "frame++\n0 0 64 64 2 1 0 0 1 2000 2000 2000 2000 2000 2000 2000 \n"
REFUSED = {
    "extra_marker": GOOD + "frame++\n",                                      # frames = 1
    "cu_before_marker": "0 0 8 8 2 1 0 0 1 2000 2000 2000 2000 2000 2000 2000 \n" + GOOD,
    "short_line": "frame++\n0 0 64 64 2 1 0 0 1 2000 2000\n",
    "long_line": "frame++\n0 0 64 64 2 1 0 0 1 2000 2000 2000 2000 2000 2000 2000 7\n",
    "not_int": "frame++\n0 0 64 64 2 1 0 0 1 2000 2000 2000 2000 2000 x 2000 \n",
    "negative": "frame++\n-4 0 64 64 2 1 0 0 1 2000 2000 2000 2000 2000 2000 2000 \n",
    "double_space": "frame++\n0  0 64 64 2 1 0 0 1 2000 2000 2000 2000 2000 2000 2000 \n",
    "empty_line": GOOD + "\n",
    "qt_too_deep": "frame++\n0 0 4 4 12 6 0 0 1 1 1 1 1 1 2000 2000 \n",
    "bt_outside_u8": "frame++\n0 0 64 64 2 1 256 0 1 2000 2000 2000 2000 2000 2000 2000 \n",
}


@pytest.mark.parametrize("name", sorted(REFUSED))
def test_dump_parser_refusals_write_nothing(lib, tmp_path, name):
    p = tmp_path / "d.txt"
    p.write_text(REFUSED[name])
    import ctypes as C
    q = np.full((1, 8, 8), 0xAB, np.uint8); b = np.full((1, 16, 16), 0xAB, np.uint8); d = np.full((1, 3, 16, 16), 0x55, np.int8)
    unk = C.c_int64(-9)
    rc = lib.pmp_read_depth_dump(str(p).encode(), 1, 64, 64, 0, q.ctypes.data, b.ctypes.data, d.ctypes.data, C.byref(unk))
    assert rc == -1, name
    assert (q == 0xAB).all() and (b == 0xAB).all() and (d == 0x55).all() and unk.value == -9


def test_dump_parser_accepts_good_and_io_error(lib, tmp_path):
    p = tmp_path / "d.txt"
    p.write_text(GOOD)
    q, b, d = engine.output_block_partition_map(str(p), 64, 64, 1)
    assert (q == 1).all() and (b == 0).all() and (d == 0).all()      # s[qtDepth] = 2000: no MTT split
    with pytest.raises(_lib.PmpError) as e:
        engine.output_block_partition_map(str(tmp_path / "missing.txt"), 64, 64, 1)
    assert e.value.code == -4


def test_restatement_equals_reference(g11):
    """Wherever the reference finished, the restatement gives its labels and a clear status; where it raised, status bit 1."""
    for name, cf, (qt, bt, dire) in K.label_sets():
        if name in ("wrap",):
            idx = g11["wrap_idx"]
            assert len(idx) >= 1
            qt, bt, dire = qt[idx], bt[idx], dire[idx]
            ref, raised = g11["wrap_msbt"][idx], g11["wrap_raised"][idx]
        else:
            ref, raised = g11[name + "_msbt"], g11[name + "_raised"]
        budget = K.BUDGET if name != "overbudget" else 10 ** 6
        m, st = K.restate_batch(qt, bt, dire, cf, budget=budget)
        fin = ~raised
        assert np.array_equal(m[fin], ref[fin]), name
        assert np.all(st[fin] & (K.INCONSISTENT | K.OVER_BUDGET) == 0), name
        assert np.all(st[raised] & K.INCONSISTENT), name
        if name == "qtdeep":
            assert np.all(st & K.QT_DEEP)
    assert g11["noisy_raised"].sum() > 20


def test_restatement_budget_and_carry_down():
    """The budget stops a region at its (budget+1)-th leaf; the best of the scored leaves stands (bit 4).  A best leaf above depth 3
    carries its deepest map down (bit 1)."""
    qt, bt, dire = K.over_budget_blocks()
    stats = []
    m_all, st_all = K.restate(qt[0], bt[0], dire[0], 1, budget=10 ** 6, stats=stats)
    assert max(stats) > K.BUDGET and st_all == 0
    m_cut, st_cut = K.restate(qt[0], bt[0], dire[0], 1)
    assert st_cut & K.OVER_BUDGET
    # noisy block that raises in the reference: its carried-down maps are monotone in depth
    qt, bt, dire = K.noisy_blocks(40, K.SEEDS["noisy"])
    m, st = K.restate_batch(qt, bt, dire, 1)
    assert np.any(st & K.INCONSISTENT)
    assert np.all(m[:, 0] <= m[:, 1]) and np.all(m[:, 1] <= m[:, 2])


def _run_cli(argv):
    from pmp_vvc_tip2023_amd import gen_labels
    return gen_labels.main(argv)


def test_cli_refuses_before_gpu(tmp_path, monkeypatch):
    """Bad flags and missing dumps exit with 2 before an Engine is created."""
    from pmp_vvc_tip2023_amd import gen_labels

    def no_gpu(*a, **k):
        raise AssertionError("GPU touched")
    monkeypatch.setattr(gen_labels.E, "Engine", no_gpu)
    d = tmp_path / "dumps"
    table = K.write_pipe_dir(str(d))
    out = str(tmp_path / "out")
    base = ["--depthDir", str(d), "--seqTable", table, "--outDir", out]
    for extra in (["--qps", "22,x"], ["--comps", "Luma,Cb"], ["--ssRatio", "0"], ["--qps", "27"]):   # QP 27 has no dumps
        with pytest.raises(SystemExit) as e:
            _run_cli(base + extra)
        assert e.value.code == 2, extra
    with pytest.raises(SystemExit) as e:
        _run_cli(base[:1] + [str(tmp_path / "nope")] + base[2:])
    assert e.value.code == 2
    with pytest.raises(SystemExit) as e:
        _run_cli(base + ["--chromaFactor", "3"])
    assert e.value.code == 2
    os.remove(os.path.join(str(d), "SeqB_QP37_Chroma_Partition_FastOff_LFNST0.txt"))
    with pytest.raises(SystemExit) as e:
        _run_cli(base + ["--qps", "22,37"])
    assert e.value.code == 2
    assert not os.path.exists(out)


def test_cli_finds_both_dump_names(tmp_path):
    from pmp_vvc_tip2023_amd import gen_labels
    d = tmp_path / "dumps"
    K.write_pipe_dir(str(d))
    assert gen_labels.find_dump(str(d), "SeqA", 22, "Luma").endswith("SeqA_QP22_Luma_Partition.txt")
    assert gen_labels.find_dump(str(d), "SeqB", 37, "Chroma").endswith("SeqB_QP37_Chroma_Partition_FastOff_LFNST0.txt")
    assert gen_labels.find_dump(str(d), "SeqC", 22, "Luma") is None


def test_engine_refuses_values_outside_reference_dtypes():
    with pytest.raises(ValueError):
        engine._fit(np.array([-1, 3]), np.uint8, "qt_map")
    with pytest.raises(ValueError):
        engine._fit(np.array([256]), np.uint8, "bt_map")
    with pytest.raises(ValueError):
        engine._fit(np.array([0.5]), np.int8, "dire_map")
    assert engine._fit(np.array([-1, 1], np.int64), np.int8, "dire_map").dtype == np.int8
