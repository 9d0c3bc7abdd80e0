"""GPU: the labels' own partition (include/pmp.h: pmp_label_partition) bit-exact with the reference-made G13
(tests/golden/g13_label_partition.npz; inputs rebuilt by tests/msbt_cases.py) and, on the over-budget block, with the numpy restatement
(tests/label_partition_cases.py); every entry point; and the driver path down to the PartitionMat file.  About 530 blocks in all."""
import os

import numpy as np
import pytest

from conftest import golden
import gpu_rig
import label_partition_cases as LP
import msbt_cases as K

pytestmark = pytest.mark.gpu

ORDER = ("valid_cf1", "valid_cf2", "noisy", "ties", "ties_cf2", "qtdeep", "bigtree_cf1", "bigtree_cf2", "overbudget")

eng = gpu_rig.engine_fixture()


@pytest.fixture(scope="module")
def g13():
    return golden("g13_label_partition.npz")


@pytest.fixture(scope="module")
def sets():
    """{name: (cf, (qt, bt, dire), restated hor, ver, status)}: computed once, shared, never written to."""
    return LP.restated_sets()


@pytest.fixture(scope="module")
def gpu(eng, sets):
    """Every set through the kernel: the chroma factor is a launch argument, so one launch per factor over the concatenated sets of
    that factor -> {name: (hor, ver, status)}."""
    out = {}
    for cf in (1, 2):
        names = [n for n in ORDER if sets[n][0] == cf]
        qt, bt, dire = (np.concatenate([sets[n][1][k] for n in names]) for k in range(3))
        hor, ver, st = eng.label_partition(qt, bt, dire, cf)
        o = 0
        for n in names:
            m = len(sets[n][1][0])
            out[n] = (hor[o:o + m], ver[o:o + m], st[o:o + m])
            o += m
    return out


def dev(*arrays):
    import torch
    return [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrays]


def run_device(eng, cf, qt, bt, dire, fill=0xFF):
    import torch
    n = len(qt)
    d = dev(qt, bt, dire)
    hor = torch.full((n, 16, 16), fill, dtype=torch.uint8, device="cuda"); ver = torch.full((n, 16, 16), fill, dtype=torch.uint8, device="cuda")
    st = torch.full((n,), fill, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    eng.label_partition_device(cf, d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), n, hor.data_ptr(), ver.data_ptr(), st.data_ptr())
    eng.synchronize()
    return hor.cpu().numpy(), ver.cpu().numpy(), st.cpu().numpy()


# ------------------------------------------------------------------------------------------------ parity
def test_kernel_equals_reference(gpu, sets, g13):
    """hor, ver bit-exact with the reference's on every set; on `overbudget` (the reference scores all 8184 leaves of a region, the
    library the first 4096) with the restatement, which defines that result."""
    assert sum(len(gpu[n][2]) for n in ORDER) == 529
    for name in ORDER:
        hor, ver, st = gpu[name]
        cf, _, rh, rv, rst = sets[name]
        eh, ev = (rh, rv) if name == "overbudget" else (g13[name + "_hor"], g13[name + "_ver"])
        assert np.array_equal(hor, eh), (name, np.nonzero(np.any(hor != eh, axis=(1, 2)))[0])
        assert np.array_equal(ver, ev), (name, np.nonzero(np.any(ver != ev, axis=(1, 2)))[0])
        assert np.array_equal(st, rst), (name, st, rst)
        if name == "qtdeep":
            assert st.any() and np.all((st == LP.QT_DEEP) | (st == 0))
        elif name == "overbudget":
            assert np.all(st == LP.OVER_BUDGET)
        else:
            assert not st.any(), name
        assert not np.any(st & K.INCONSISTENT)            # bit 1 is never set on this path


def test_cases_each_set_exists_for(gpu, sets):
    for name in ("valid_cf1", "valid_cf2"):
        hor, ver, st = gpu[name]
        qt, bt, dire = sets[name][1]
        split = qt[:, 0, 0] >= 1
        # row 8 and column 8 belong to the lower / right quadrants' waves; wave 0 paints them (the depth-0 cross) and the upper /
        # left quadrants' CUs end on them
        assert split.sum() > 20 and np.all(hor[split, 8, :] == 1) and np.all(ver[split, :, 8] == 1)
        whole = ~split                                    # one 64x64 QT leaf: waves 1..3 paint nothing and must hand over zeros
        assert whole.sum() > 5
        assert np.all(hor[whole, 0, :] == 1) and np.all(ver[whole, :, 0] == 1)
        assert np.array_equal(hor[whole], sets[name][2][whole]) and np.array_equal(ver[whole], sets[name][3][whole])
    # best leaves above depth 3 (noisy): the restated search finds some, and the kernel painted exactly their CUs
    cf, (qt, bt, dire), rh, rv, _ = sets["noisy"]
    shallow = [i for i in range(len(qt)) if qt[i, 0, 0] == 0 and LP.region_cus(bt[i], dire[i], cf, 0, 0, 16, 16)[1] < 3]
    assert len(shallow) >= 3
    assert np.array_equal(gpu["noisy"][0][shallow], rh[shallow]) and np.array_equal(gpu["noisy"][1][shallow], rv[shallow])
    # first-minimum ties at both factors: a tie broken the other way would flip hor and ver
    for name in ("ties", "ties_cf2"):
        assert np.array_equal(gpu[name][0], sets[name][2]) and np.array_equal(gpu[name][1], sets[name][3])
        assert np.any(gpu[name][0] != gpu[name][1].transpose(0, 2, 1))
    # crosses at depth 3 under qt 4..6: quadrant 0 is deep in every qtdeep block
    hor, ver, st = gpu["qtdeep"]
    assert set(np.unique(sets["qtdeep"][1][0])) >= {4, 5, 6}
    assert np.all(hor[:, 1, 0:2] == 1) and np.all(ver[:, 0:2, 1] == 1) and np.all(st & LP.QT_DEEP)


# ------------------------------------------------------------------------------------------------ API forms
def test_host_device_records_and_prefill(eng, gpu, sets):
    import torch
    from pmp_vvc_tip2023_amd import _lib
    cf, (qt, bt, dire) = sets["noisy"][:2]
    h0, v0, s0 = gpu["noisy"]
    for fill in (0xFF, 0x00):                             # every output byte is written, whatever was there
        h1, v1, s1 = run_device(eng, cf, qt, bt, dire, fill)
        assert np.array_equal(h1, h0) and np.array_equal(v1, v0) and np.array_equal(s1, s0)
    n = len(qt)
    d = dev(qt, bt, dire)
    rec = torch.full((n, _lib.PMP_RECORD_BYTES), 0xFF, dtype=torch.uint8, device="cuda"); st = torch.full((n,), 0xFF, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    eng.label_partition_records_device(cf, d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), n, rec.data_ptr(), st.data_ptr())
    eng.synchronize()
    r = rec.cpu().numpy()
    assert np.array_equal(r[:, :256].reshape(n, 16, 16), h0) and np.array_equal(r[:, 256:512].reshape(n, 16, 16), v0)
    assert np.array_equal(r[:, 512:576], qt.reshape(n, 64)) and np.array_equal(r[:, 576:].view(np.int8), dire.reshape(n, 768))
    assert np.array_equal(st.cpu().numpy(), s0)


def test_one_block_chunks_and_repeat(eng, gpu, sets):
    cf, (qt, bt, dire) = sets["qtdeep"][:2]
    h0, v0, s0 = gpu["qtdeep"]
    h, v, s = eng.label_partition(qt[3:4], bt[3:4], dire[3:4], cf)          # n = 1
    assert np.array_equal(h, h0[3:4]) and np.array_equal(v, v0[3:4]) and np.array_equal(s, s0[3:4])
    h1, v1, s1 = eng.label_partition(qt[:9], bt[:9], dire[:9], cf)
    eng.set_chunk(4)                                      # n = 9 in passes of 4, 4, 1
    try:
        h2, v2, s2 = eng.label_partition(qt[:9], bt[:9], dire[:9], cf)
    finally:
        eng.set_chunk(4096)
    for a, b, c in ((h1, h2, h0), (v1, v2, v0), (s1, s2, s0)):
        assert np.array_equal(a, b) and np.array_equal(a, c[:9])
    # the same inputs give the same bits
    a = run_device(eng, cf, qt, bt, dire)
    b = run_device(eng, cf, qt, bt, dire)
    assert all(np.array_equal(x, y) for x, y in zip(a, b)) and np.array_equal(a[0], h0)


def test_empty_and_refusals(eng, sets):
    import torch
    from pmp_vvc_tip2023_amd import _lib
    cf, (qt, bt, dire) = sets["ties"][:2]
    h, v, s = eng.label_partition(qt[:0], bt[:0], dire[:0], 1)
    assert h.shape == (0, 16, 16) and v.shape == (0, 16, 16) and s.shape == (0,)
    d = dev(qt, bt, dire)
    n = len(qt)
    hor = torch.full((n * 256 + 4,), 0xFF, dtype=torch.uint8, device="cuda"); ver = torch.full((n * 256,), 0xFF, dtype=torch.uint8, device="cuda")
    rec = torch.full((n * _lib.PMP_RECORD_BYTES + 4,), 0xFF, dtype=torch.uint8, device="cuda"); st = torch.full((n,), 0xFF, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    p = [t.data_ptr() for t in d]
    # n = 0: nothing is launched, nothing is written - with buffers and without
    eng.label_partition_device(1, p[0], p[1], p[2], 0, hor.data_ptr(), ver.data_ptr(), st.data_ptr())
    eng.label_partition_records_device(2, p[0], p[1], p[2], 0, rec.data_ptr(), st.data_ptr())
    eng.label_partition_device(2, 0, 0, 0, 0, 0, 0, 0)
    eng.label_partition_records_device(1, 0, 0, 0, 0, 0, 0)

    def invalid(fn, *a):
        with pytest.raises(_lib.PmpError) as e:
            fn(*a)
        assert e.value.code == -1
    invalid(eng.label_partition_device, 3, p[0], p[1], p[2], n, hor.data_ptr(), ver.data_ptr(), st.data_ptr())
    invalid(eng.label_partition_records_device, 0, p[0], p[1], p[2], n, rec.data_ptr(), st.data_ptr())
    invalid(eng.label_partition_device, 1, p[0], p[1], p[2], n, hor.data_ptr() + 1, ver.data_ptr(), st.data_ptr())
    invalid(eng.label_partition_device, 1, p[0], p[1] + 2, p[2], n, hor.data_ptr(), ver.data_ptr(), st.data_ptr())
    invalid(eng.label_partition_records_device, 1, p[0], p[1], p[2], n, rec.data_ptr() + 2, st.data_ptr())
    invalid(eng.label_partition_device, 1, p[0], p[1], p[2], -1, hor.data_ptr(), ver.data_ptr(), st.data_ptr())
    invalid(eng.label_partition_device, 1, p[0], 0, p[2], n, hor.data_ptr(), ver.data_ptr(), st.data_ptr())
    eng.synchronize()
    for t in (hor, ver, rec, st):                         # none of the calls above wrote a byte
        assert bool((t == 0xFF).all())
    with pytest.raises(ValueError):
        eng.label_partition(qt, bt, dire, 3)


def test_labels_path_unchanged(eng, sets):
    """pmp_msbt_labels shares the search with the new kernel: on the same inputs it still gives the reference's labels (G11)."""
    g11 = golden("g11_msbt.npz")
    for name in ("valid_cf2", "ties", "bigtree_cf1"):
        cf, (qt, bt, dire) = sets[name][:2]
        m, st = eng.gen_seq_sub_map(qt, bt, dire, is_luma=(cf == 1), return_status=True)
        assert not g11[name + "_raised"].any() and not st.any()
        assert np.array_equal(m, g11[name + "_msbt"]), name


# ------------------------------------------------------------------------------------------------ driver path
def expected_text(g13, seq, comp, qp, frames, h, w):
    return LP.map_255_to_minus1(g13[LP.pipe_key(seq, comp, qp) + "text"].tobytes().decode(), frames, h, w)[0]


def test_engine_writes_the_reference_file(eng, g13, tmp_path):
    from pmp_vvc_tip2023_amd import engine
    K.write_pipe_dir(str(tmp_path))
    for seq, comp, qp, w, h, frames in LP.pipe_cases():
        q8, bt, dire = engine.output_block_partition_map(LP.pipe_dump_path(str(tmp_path), seq, comp, qp), w, h, frames, 64, comp == "Chroma")
        txt, binp = str(tmp_path / "o.txt"), str(tmp_path / "o.pmpb")
        hor, ver, st = eng.label_partition_for_VTM(q8 - np.uint8(1), bt, dire, comp == "Luma", txt, frames, w, h)
        assert not st.any()
        assert open(txt).read() == expected_text(g13, seq, comp, qp, frames, h, w), (seq, comp, qp)
        eng.label_partition_for_VTM(q8 - np.uint8(1), bt, dire, comp == "Luma", binp, frames, w, h, binary=True)
        f2, h2, w2, bh, bv, bq, bd = engine.read_partition_binary(binp)
        th, tv, tq, td = engine.read_partition_file(txt, frames, h, w)
        assert (f2, h2, w2) == (frames, h, w)
        assert np.array_equal(bh, th) and np.array_equal(bv, tv) and np.array_equal(bq, tq) and np.array_equal(bd, td)
    with pytest.raises(ValueError):
        eng.label_partition_for_VTM(q8 - np.uint8(1), bt, dire, True, None, frames + 1, w, h)


def test_cli_writes_the_files(g13, tmp_path):
    from pmp_vvc_tip2023_amd import engine, label_partition
    table = K.write_pipe_dir(str(tmp_path / "dumps"))
    base = ["--depthDir", str(tmp_path / "dumps"), "--seqTable", table, "--qps", ",".join(str(q) for q in K.PIPE_QPS),
            "--ssRatio", str(K.PIPE_SS)]
    out, outb = str(tmp_path / "out"), str(tmp_path / "outb")
    assert label_partition.main(base + ["--outDir", out]) == 0
    assert label_partition.main(base + ["--outDir", outb, "--binary", "--comps", "Chroma"]) == 0
    for seq, comp, qp, w, h, frames in LP.pipe_cases():
        path = os.path.join(out, "PartitionMat", "%s_%s_QP%d_PartitionMat.txt" % (seq, comp, qp))
        assert open(path).read() == expected_text(g13, seq, comp, qp, frames, h, w), (seq, comp, qp)
        pb = os.path.join(outb, "PartitionMat", "%s_%s_QP%d_PartitionMat.pmpb" % (seq, comp, qp))
        assert os.path.isfile(pb) == (comp == "Chroma")
        if comp == "Chroma":
            got = engine.read_partition_binary(pb)[3:]
            want = engine.read_partition_file(path, frames, h, w)
            assert all(np.array_equal(a, b) for a, b in zip(got, want))
    assert len(os.listdir(os.path.join(out, "PartitionMat"))) == 8


def test_cli_flagged_sequence(tmp_path, capsys):
    """A dump with qtDepth 5 gives qt = 4 at every depth-3 node (status bit 2): no file and exit 3, unless --keepFlagged."""
    from pmp_vvc_tip2023_amd import engine, label_partition
    d = tmp_path / "dumps"
    d.mkdir()
    (d / "Deep_QP32_Luma_Partition.txt").write_text("frame++\n0 0 64 64 10 5 0 0 1 1 1 1 1 2000 2000 2000 \n")
    (d / "Fine_QP32_Luma_Partition.txt").write_text("frame++\n0 0 64 64 2 1 0 0 1 2000 2000 2000 2000 2000 2000 2000 \n")
    table = d / "seqs.txt"
    table.write_text("Deep,Deep.yuv,64,64,1,30\nFine,Fine.yuv,64,64,1,30\n")
    base = ["--depthDir", str(d), "--seqTable", str(table), "--qps", "32", "--comps", "Luma"]
    out = tmp_path / "out"
    assert label_partition.main(base + ["--outDir", str(out)]) == 3
    assert os.listdir(str(out / "PartitionMat")) == ["Fine_Luma_QP32_PartitionMat.txt"]
    assert "Deep Luma QP32: 1 blocks, cf 1, unknown split codes 0; status bit2 (qt > 3) 1, bit4 (leaf budget) 0" in capsys.readouterr().out
    out2 = tmp_path / "out2"
    assert label_partition.main(base + ["--outDir", str(out2), "--keepFlagged"]) == 0
    hor, ver, qt, dire = engine.read_partition_file(str(out2 / "PartitionMat" / "Deep_Luma_QP32_PartitionMat.txt"), 1, 64, 64)
    # crosses of depths 0..3 cover every row and column but the first; nothing else is painted
    assert np.all(qt == 4) and np.all(hor[0, 1:, :] == 1) and np.all(hor[0, 0, :] == 0) and np.all(ver[0, :, 1:] == 1) and np.all(ver[0, :, 0] == 0)
    hor, ver, qt, dire = engine.read_partition_file(str(out2 / "PartitionMat" / "Fine_Luma_QP32_PartitionMat.txt"), 1, 64, 64)
    assert np.all(qt == 0) and hor[0].sum() == 16 and np.all(hor[0, 0, :] == 1) and np.all(ver[0, :, 0] == 1)
