"""CPU: what tests/test_gpu_dataset.py stands on, and everything of make_dataset that needs no GPU.

dataset_cases' numpy cutter equals CreateDataSet.output_block_yuv (g21_dataset.npz: 192x136, 33 frames at ratio 8, 8 and 10 bits, cut
by the reference) and Inference_QBD's copy of it (g6_cut.npz, on that golden's planes); its select and gather restatements hold their
contract on small hand-made cases; make_dataset.plan refuses a missing YUV, a wrong file size, a bad --bitDepth, a negative --maxPerSeq
and a missing dump with exit status 2 and never constructs an Engine; `make traincheck` passes with the two new refusal functions in
its matrix; the library exports both calls."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT, golden
import dataset_cases as K
import msbt_cases as M

CSRC = os.path.join(ROOT, "pmp_vvc_tip2023_amd", "csrc")


def test_the_cutter_restatement_equals_the_reference_on_g21():
    g = np.load(K.GOLDEN, allow_pickle=False)
    assert os.path.getsize(K.GOLDEN) < 1000000
    c = K.G21
    for bits in (8, 10):
        y, u, v = K.yuv_planes(c["width"], c["height"], c["frames"], bits, c["seed"])
        by, bu, bv = K.cut(y, u, v, bits, c["ss"])
        assert by.shape == (30, 68, 68) and bu.shape == (30, 34, 34)
        for got, key in ((by, "by"), (bu, "bu"), (bv, "bv")):
            want = g["%s%d" % (key, bits)]
            assert want.dtype == np.uint8 and np.array_equal(got, want), (key, bits)
    assert K.block_rows([(192, 136, 33)], 8).shape == (30, 4) and K.block_rows([(192, 136, 33)], 8)[-1].tolist() == [0, 4, 1, 2]


def test_the_cutter_restatement_equals_g6_on_its_planes():
    g = golden("g6_cut.npz")
    for bits in (8, 10):
        by, bu, bv = K.cut(g["y%d" % bits], g["u%d" % bits], g["v%d" % bits], bits)
        assert np.array_equal(by, g["by%d" % bits]) and np.array_equal(bu, g["bu%d" % bits]) and np.array_equal(bv, g["bv%d" % bits])


def test_the_written_file_reads_back_as_its_planes(tmp_path):
    from pmp_vvc_tip2023_amd.inference_qbd import import_yuv420
    for bits in (8, 10):
        p = str(tmp_path / ("s%d.yuv" % bits))
        y, u, v = K.write_yuv(p, 128, 64, 9, bits, 5)
        assert os.path.getsize(p) == 128 * 64 * 3 // 2 * 9 * (2 if bits == 10 else 1)
        yy, uu, vv = import_yuv420(p, 128, 64, 9, 8, bits == 10)
        assert np.array_equal(yy, y[::8]) and np.array_equal(uu, u[::8]) and np.array_equal(vv, v[::8])


def test_select_and_gather_restatements_on_hand_made_cases():
    f = [np.array([0, 1, 2, 0, 4, 0, 0, 8], np.uint8), np.array([0, 0, 0, 4, 0, 0, 2, 0], np.uint8)]
    index, count = K.select(f, 5, [3, 3, 8], 0, 8)            # candidates: 0, 2 | | 5, 6, 7
    assert index.tolist() == [0, 2, 5, 6, 7, -1, -1, -1] and count.tolist() == [2, 0, 3, 5]
    index, count = K.select(f, 5, [3, 3, 8], 2, 8)
    assert index.tolist() == [0, 2, 5, 6, -1, -1, -1, -1] and count.tolist() == [2, 0, 2, 4]
    index, count = K.select([], 5, [8], 3, 8)
    assert index.tolist() == [0, 1, 2, -1, -1, -1, -1, -1] and count.tolist() == [3, 3]
    src = np.arange(12, dtype=np.int32).reshape(4, 3)
    out, status = K.gather(src, [3, 3, 0])
    assert out.tolist() == [[9, 10, 11], [9, 10, 11], [0, 1, 2]] and status == 0
    out, status = K.gather(src, [1, -1, 4, 2])
    assert out.tolist() == [[3, 4, 5], [0, 0, 0], [0, 0, 0], [6, 7, 8]] and status == 1
    for n in K.SELECT_N:
        for name, seg in K.segment_lists(n).items():
            assert seg[-1] == n and all(a <= b for a, b in zip(seg, seg[1:])), (n, name)
    assert [int(np.count_nonzero(a & 5)) for a in K.flag_arrays("last", 3, 65, 1)] == [1, 1, 1]
    assert all((a & 5).all() for a in K.flag_arrays("all", 3, 65, 1)) and not any((a & 5).any() for a in K.flag_arrays("none", 3, 65, 1))


# ---- make_dataset.plan
@pytest.fixture()
def pipe(tmp_path):
    """msbt_cases' dump directory with its two sequences' YUV files beside it -> (the command's arguments, the directory)"""
    d = str(tmp_path / "in")
    table = M.write_pipe_dir(d)
    for i, (name, w, h, f) in enumerate(M.PIPE_SEQS):
        K.write_yuv(os.path.join(d, name + ".yuv"), w, h, f, 8, 40 + i)
    argv = ["--seqDir", d, "--depthDir", d, "--seqTable", table, "--outDir", str(tmp_path / "out"), "--dataType", "Train", "--qps", "22,37"]
    return argv, d


def refused(argv, capsys, monkeypatch, word):
    from pmp_vvc_tip2023_amd import engine, make_dataset

    def no_engine(*a, **k):
        raise AssertionError("an Engine was constructed")
    monkeypatch.setattr(engine, "Engine", no_engine)
    with pytest.raises(SystemExit) as e:
        make_dataset.main(argv)
    err = capsys.readouterr().err
    assert e.value.code == 2 and err.startswith("make_dataset: ") and word in err, err
    assert not os.path.exists(argv[argv.index("--outDir") + 1])


def test_plan_accepts_the_pipeline_case_and_finds_every_file(pipe):
    from pmp_vvc_tip2023_amd import make_dataset
    argv, d = pipe
    qps, comps, seqs, dumps = make_dataset.plan(make_dataset.build_parser().parse_args(argv))
    assert qps == [22, 37] and comps == ["Luma", "Chroma"] and len(dumps) == 8 and all(os.path.isfile(p) for p in dumps.values())
    assert [(s["name"], s["width"], s["height"], s["frames"], s["sub"], s["is10bit"]) for s in seqs] == \
        [("SeqA", 256, 128, 9, 2, False), ("SeqB", 192, 192, 4, 1, False)]
    assert seqs[0]["path"] == os.path.join(d, "SeqA.yuv")


def test_plan_reads_path_and_bit_depth_from_a_cfg(pipe, tmp_path):
    from pmp_vvc_tip2023_amd import make_dataset
    argv, d = pipe
    cfg = tmp_path / "cfg"
    cfg.mkdir()
    K.write_yuv(os.path.join(d, "SeqB_10bit.yuv"), 192, 192, 4, 10, 41)
    (cfg / "SeqA.cfg").write_text("InputFile : SeqA.yuv   # relative: looked for in --seqDir\nInputBitDepth : 8\n")
    (cfg / "SeqB.cfg").write_text("InputFile : %s\nInputBitDepth : 10\n" % os.path.join(d, "SeqB_10bit.yuv"))
    _, _, seqs, _ = make_dataset.plan(make_dataset.build_parser().parse_args(argv + ["--cfgDir", str(cfg)]))
    assert [s["is10bit"] for s in seqs] == [False, True] and seqs[1]["path"].endswith("SeqB_10bit.yuv") and seqs[0]["path"] == os.path.join(d, "SeqA.yuv")


def test_plan_refuses_a_missing_yuv(pipe, capsys, monkeypatch):
    argv, d = pipe
    os.remove(os.path.join(d, "SeqB.yuv"))
    refused(argv, capsys, monkeypatch, "SeqB.yuv not found")


def test_plan_refuses_a_wrong_file_size(pipe, capsys, monkeypatch):
    argv, d = pipe
    with open(os.path.join(d, "SeqA.yuv"), "ab") as fp:
        fp.write(b"\0")
    refused(argv, capsys, monkeypatch, "needs %d" % (256 * 128 * 3 // 2 * 9))


def test_plan_refuses_8_bit_files_read_as_10_bit(pipe, capsys, monkeypatch):
    refused(pipe[0] + ["--bitDepth", "10"], capsys, monkeypatch, "at 10 bits needs")


def test_plan_refuses_a_bad_bit_depth(pipe, capsys, monkeypatch):
    refused(pipe[0] + ["--bitDepth", "12"], capsys, monkeypatch, "--bitDepth")


def test_plan_refuses_a_negative_cap(pipe, capsys, monkeypatch):
    refused(pipe[0] + ["--maxPerSeq", "-1"], capsys, monkeypatch, "--maxPerSeq")


def test_plan_refuses_a_missing_dump(pipe, capsys, monkeypatch):
    argv, d = pipe
    os.remove(os.path.join(d, "SeqA_QP37_Chroma_Partition.txt"))
    refused(argv, capsys, monkeypatch, "missing dump")


# ---- the native side
def test_train_check_passes_with_the_data_set_matrix():
    """train_check.h with a main of its own under AddressSanitizer and UBSan: a stand-alone CPU program, built and run once."""
    r = subprocess.run(["make", "-s", "-C", CSRC, "traincheck"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "train_check: ok" in r.stdout, (r.stdout + r.stderr)[-2000:]
    main = open(os.path.join(CSRC, "train_check_main.cpp")).read()
    assert "select_refused(" in main and "rows_gather_refused(" in main
    api = open(os.path.join(CSRC, "api_dataset.cpp")).read()
    assert "select_refused(" in api and "rows_gather_refused(" in api, "the entry points refuse through the same functions"


def test_the_library_exports_both_calls_and_the_engine_binds_them():
    from pmp_vvc_tip2023_amd import _lib, engine
    lib = _lib.load()
    assert hasattr(lib, "pmp_select_rows_device") and hasattr(lib, "pmp_gather_rows_device")
    assert len(_lib.SIGNATURES["pmp_select_rows_device"][1]) == 10 and len(_lib.SIGNATURES["pmp_gather_rows_device"][1]) == 8
    hdr = open(os.path.join(ROOT, "include", "pmp.h")).read()
    assert "#define PMP_SELECT_MAX_FLAGS %d\n" % _lib.PMP_SELECT_MAX_FLAGS in hdr
    for name in ("select_rows_device", "gather_rows_device", "select_rows", "gather_rows"):
        assert callable(getattr(engine.Engine, name)), name
    assert "dataset" in open(os.path.join(CSRC, "Makefile")).read()
