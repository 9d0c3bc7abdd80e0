"""GPU: the driver's two block sources x two emission paths write the same bytes, and the Stages accounting keeps its contract.

One job of two tiny sequences - 3 frames of 192x128 (6 blocks each) and a 96x48 one without a full block - over Luma, Chroma x QP 22, 37:
four passes per sequence, so both slots of the sharded sink's record buffer are reused, and the second sequence takes the
zero-block path in every mode."""
import os
import time

import pytest

pytestmark = pytest.mark.gpu

MODES = {"default": [], "hostBlocks": ["--hostBlocks"], "gather": ["--emit", "gather"], "hostBlocks-gather": ["--hostBlocks", "--emit", "gather"]}
NAMES = ("setup", "weights", "read_wait", "h2d_cut", "first_enqueue", "gpu_wait", "enqueue", "d2h", "emit_start", "emit_finish", "gather", "drain", "teardown")


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    from pmp_vvc_tip2023_amd import synth
    root = tmp_path_factory.mktemp("driver_matrix")
    inp = root / "in"
    inp.mkdir()
    y, u, v = synth.recipe_r_frames(3, 128, 192, 23)
    with open(inp / "SeqA_192x128_30.yuv", "wb") as f:
        for i in range(3):
            f.write(y[i].tobytes()); f.write(u[i].tobytes()); f.write(v[i].tobytes())
    (inp / "Small_96x48_30.yuv").write_bytes(bytes(2 * 96 * 48 * 3 // 2))
    (inp / "table.txt").write_text("SeqA,SeqA_192x128_30.yuv,192,128,3,30\nSmall,Small_96x48_30.yuv,96,48,2,30\n#end!!!!\n")
    (inp / "SeqA.cfg").write_text("InputFile : SeqA_192x128_30.yuv\nInputBitDepth : 8\n")
    (inp / "Small.cfg").write_text("InputFile : Small_96x48_30.yuv\nInputBitDepth : 8\n")
    return root


def run_job(root, mode):
    """The job in-process in one mode: ({file name: bytes}, the Time_Sta text, the run's Stages, the wall time of D.main)."""
    from pmp_vvc_tip2023_amd import inference_qbd as D
    inp, out = root / "in", root / ("out_" + mode)
    t0 = time.perf_counter()
    D.main(["--jobID", "m", "--inputDir", str(inp), "--outDir", str(out), "--seqTable", "table.txt", "--cfgDir", str(inp), "--ssRatio", "1",
            "--startSeqID", "0", "--seqNum", "2", "--qps", "22,37", "--binary", "--allowSyntheticMTT"] + MODES[mode])
    wall = time.perf_counter() - t0
    pm = out / "m" / "PartitionMat"
    files = {n: open(pm / n, "rb").read() for n in sorted(os.listdir(pm))}
    return files, open(out / "m" / "Time_Sta_0_2.txt").read(), D.LAST_STAGES, wall


@pytest.fixture(scope="module")
def default_run(inputs):
    return run_job(inputs, "default")


@pytest.mark.parametrize("mode", list(MODES))
def test_every_driver_mode_writes_the_same_files(inputs, default_run, mode):
    files, sta, _, _ = default_run if mode == "default" else run_job(inputs, mode)
    want = sorted("%s_%s_QP%d_PartitionMat.%s" % (stem, comp, qp, ext) for stem in ("SeqA_192x128_30", "Small_96x48_30")
                  for comp in ("Luma", "Chroma") for qp in (22, 37) for ext in ("txt", "pmpb"))
    assert sorted(files) == want and len(want) == 8 + 8
    for n in want:
        assert files[n] == default_run[0][n], (mode, n)
    # not vacuous: 3 frames of 32 x 48 cells (five matrices, one of them at half resolution) and a header-only binary beside an empty text
    assert files["SeqA_192x128_30_Luma_QP22_PartitionMat.txt"].count(b"\n") == 3 * (5 * 32 * 48 + 16 * 24)
    assert files["Small_96x48_30_Chroma_QP37_PartitionMat.txt"] == b"" and len(files["Small_96x48_30_Chroma_QP37_PartitionMat.pmpb"]) == 40
    rows = sta.strip().split("\n")
    assert len(rows) == 8 and all(r.count(",") == 5 for r in rows)


def test_stages_contract_after_the_default_run(default_run):
    """What tools/driver_bench.py reads: the 13 stage names in their order, one time each, pass and pass-block counts, and times that
    are disjoint intervals of the main thread - none negative, together no longer than the call."""
    _, _, st, wall = default_run
    assert tuple(st.NAMES) == NAMES
    assert set(st.t) == set(st.NAMES)
    assert st.passes == 8 and st.blocks == 72
    assert all(v >= 0 for v in st.t.values()) and st.prefetch_read >= 0
    assert sum(st.t.values()) <= wall
