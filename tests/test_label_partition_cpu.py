"""CPU: the numpy restatement of GenMSBtMap.map_to_parititon (tests/label_partition_cases.py) against the reference-made G13
(tests/golden/g13_label_partition.npz), the reference's PartitionMat files against the restatement through the library's host-only text
formatter, the exported symbols, and label_partition's flag, file and shape handling before any GPU work."""
import os

import numpy as np
import pytest

from conftest import golden
import label_partition_cases as LP
import msbt_cases as K
from pmp_vvc_tip2023_amd import _lib, engine


@pytest.fixture(scope="module")
def lib():
    if not os.path.isfile(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.load()


@pytest.fixture(scope="module")
def g13():
    return golden("g13_label_partition.npz")


def test_restatement_equals_reference(g13):
    """Bit for bit on every set but `overbudget`.  There the reference scores all 8184 leaves of each region; with the library's budget of
    4096 the restatement IS the definition of the result (status bit 4), so only its unbudgeted run is compared with the reference."""
    sets = LP.restated_sets()
    assert sorted(sets) == sorted(k[:-4] for k in g13.files if k.endswith("_hor"))
    for name, (cf, (qt, bt, dire), hor, ver, st) in sets.items():
        if name == "overbudget":
            assert np.all(st == LP.OVER_BUDGET)
            hor, ver, st_all = LP.restate_batch(qt, bt, dire, cf, budget=10 ** 6)
            assert not st_all.any()
        assert np.array_equal(hor, g13[name + "_hor"]), name
        assert np.array_equal(ver, g13[name + "_ver"]), name
        assert hor.max() <= 1 and ver.max() <= 1
        if name == "qtdeep":
            assert st.any() and np.all(st & ~np.uint8(LP.QT_DEEP) == 0)
        elif name != "overbudget":
            assert not st.any(), name


def test_cases_cover_what_they_exist_for():
    sets = LP.restated_sets()
    for name in ("valid_cf1", "valid_cf2"):
        cf, (qt, bt, dire), hor, ver, st = sets[name]
        split = qt[:, 0, 0] >= 1
        # QT crosses on row / column 8, and MTT edges of one quadrant's CUs that end on them: painted across wave ownership
        assert split.sum() > 20 and np.all(hor[split, 8, :] == 1) and np.all(ver[split, :, 8] == 1)
        assert (~split).sum() > 5                         # one 64x64 QT leaf: three waves paint nothing
    cf, (qt, bt, dire), hor, ver, st = sets["noisy"]
    shallow = 0
    for i in range(len(qt)):
        if qt[i, 0, 0] == 0:
            shallow += LP.region_cus(bt[i], dire[i], cf, 0, 0, 16, 16)[1] < 3
    assert shallow >= 3                                   # best leaves above depth 3: legal on this path
    cf, (qt, bt, dire), hor, ver, st = sets["qtdeep"]
    assert set(np.unique(qt)) >= {4, 5, 6}
    assert np.all(hor[:, 1, 0:2] == 1) and np.all(ver[:, 0:2, 1] == 1)      # quadrant 0 is always deep: the depth-3 cross at (0, 0)


def test_region_walks_agree():
    """region_cus walks msbt_cases.region's tree: same best depth, leaf count, stop and leaf map; its CUs tile the region."""
    for name in ("noisy", "ties_cf2", "bigtree_cf1", "overbudget"):
        cf, (qt, bt, dire) = [(c, x) for n, c, x in LP.label_sets() if n == name][0]
        for i in range(min(len(qt), 12)):
            s = 16 >> min(int(qt[i, 0, 0]), 3)
            cus, d, m, n, stop = LP.region_cus(bt[i], dire[i], cf, 0, 0, s, s)
            maps, d0, n0, stop0 = K.region(bt[i], dire[i], cf, 0, 0, s, s)
            assert (d, n, stop) == (d0, n0, stop0)
            if d > 0:
                assert np.array_equal(maps[2][:s, :s], m[:s, :s].astype(np.uint8))
            cover = np.zeros((16, 16), int)
            for (x, y, h, w) in cus:
                cover[x:x + h, y:y + w] += 1
            assert np.all(cover[:s, :s] == 1) and cover.sum() == s * s


def test_reference_files_equal_restatement_through_formatter(lib, g13, tmp_path):
    """The reference's file for every pipe sequence = pmp_format_partition_text of the restated flags with the labels as qt / direction
    sections, once the reference's '255' direction lines (its u8 cast, GenMSBtMap.py:413) read '-1' - and that is the only difference."""
    K.write_pipe_dir(str(tmp_path))
    total_changed = 0
    for seq, comp, qp, w, h, frames in LP.pipe_cases():
        q8, bt, dire = engine.output_block_partition_map(LP.pipe_dump_path(str(tmp_path), seq, comp, qp), w, h, frames, 64, comp == "Chroma")
        qt = q8 - np.uint8(1)
        hor, ver, st = LP.restate_batch(qt, bt, dire, 1 if comp == "Luma" else 2)
        assert not st.any()
        mine = engine.format_partition_text(frames, h, w, hor, ver, qt, dire).decode()
        ref = g13[LP.pipe_key(seq, comp, qp) + "text"].tobytes().decode()
        mapped, changed = LP.map_255_to_minus1(ref, frames, h, w)
        assert mapped == mine, (seq, comp, qp)
        assert changed == int(np.count_nonzero(dire == -1)) and ref.count("-") == 0
        assert (ref == mine) == (changed == 0)
        total_changed += changed
    assert total_changed > 0


def test_library_exports_the_entry_points(lib):
    for name in ("pmp_label_partition", "pmp_label_partition_device", "pmp_label_partition_records_device"):
        assert hasattr(lib, name) and name in _lib.SIGNATURES
    # no context: refused before anything else happens
    assert lib.pmp_label_partition(None, 1, None, None, None, 0, None, None, None) < 0


def test_cli_refuses_before_gpu(lib, tmp_path, monkeypatch):
    """Bad flags, missing or malformed dumps and sequences without a block exit with 2 before an Engine is created."""
    from pmp_vvc_tip2023_amd import label_partition

    def no_gpu(*a, **k):
        raise AssertionError("GPU touched")
    monkeypatch.setattr(label_partition.E, "Engine", no_gpu)
    d = tmp_path / "dumps"
    table = K.write_pipe_dir(str(d))
    out = str(tmp_path / "out")
    base = ["--depthDir", str(d), "--seqTable", table, "--outDir", out, "--qps", "22,37"]

    def refused(argv):
        with pytest.raises(SystemExit) as e:
            label_partition.main(argv)
        assert e.value.code == 2, argv
        assert not os.path.exists(out)

    for extra in (["--qps", "22,x"], ["--comps", "Luma,Cb"], ["--ssRatio", "0"], ["--qps", "27"], ["--chromaFactor", "3"],
                  ["--keepInconsistent"], ["--dataType", "Train"]):
        refused(base + extra)
    refused(base[:1] + [str(tmp_path / "nope")] + base[2:])
    refused(base[:3] + [str(tmp_path / "no_table.txt")] + base[4:])
    # wrong shapes: a table whose geometry the dump does not fit (more frame markers than ceil(frames / ssRatio)) ...
    t2 = tmp_path / "short.txt"
    t2.write_text("SeqA,SeqA.yuv,256,128,8,30\n")        # 1 dumped frame expected, the dump holds 2
    refused(base[:3] + [str(t2)] + base[4:] + ["--comps", "Luma"])
    # ... and a sequence smaller than one block
    t3 = tmp_path / "small.txt"
    t3.write_text("SeqA,SeqA.yuv,256,48,9,30\n")
    refused(base[:3] + [str(t3)] + base[4:] + ["--comps", "Luma"])
    # a malformed dump
    bad = d / "SeqB_QP37_Chroma_Partition_FastOff_LFNST0.txt"
    bad.write_text(bad.read_text() + "1 2 3\n")
    refused(base)
    os.remove(str(bad))
    refused(base)


def test_engine_method_refuses_bad_arguments_without_a_context():
    e = object.__new__(engine.Engine)                    # no context: these checks come first
    qt, bt, dire = K.valid_blocks(2, 5, 1)
    with pytest.raises(ValueError):
        engine.Engine.label_partition(e, qt, bt, dire, 3)
    with pytest.raises(ValueError):
        engine.Engine.label_partition(e, qt, bt[:1], dire, 1)
    with pytest.raises(ValueError):
        engine.Engine.label_partition(e, qt.astype(np.int16) - 1, bt, dire, 1)      # -1 does not fit u8: the caller wraps, not we
    e.h = None
