"""CPU: python -m pmp_vvc_tip2023_amd.train_qbd before it touches the GPU - plan() refuses each bad flag, missing file, wrong dtype,
wrong shape and mismatched count with status 2 and without initialising torch.cuda; the reference's flags keep their defaults; the
learning-rate rule equals Metrics.adjust_learning_rate over epochs 0..200, the 1e-6 floor that holds the old value included; an
epoch's batch order depends on (seed, epoch) alone."""
import os
import subprocess
import sys

import numpy as np
import pytest

import train_qbd_cases as TC
from conftest import ROOT
from pmp_vvc_tip2023_amd import train_qbd as T


@pytest.fixture(scope="module")
def data(tmp_path_factory):
    d = tmp_path_factory.mktemp("sets")
    TC.write_sets(str(d), "Luma", 22, n=3)
    TC.write_sets(str(d), "Chroma", 27, n=3)
    return d


def plan(argv):
    return T.plan(T.build_parser().parse_args(argv))


def refused(argv, capsys, needle):
    with pytest.raises(SystemExit) as e:
        plan(argv)
    assert e.value.code == 2
    err = capsys.readouterr().err
    assert err.startswith("train_qbd: ") and needle in err, err


def test_reference_flags_keep_their_defaults():
    a = T.build_parser().parse_args([])
    want = dict(jobID="0000", isLuma=False, inputDir="/input/", outDir="/output/", lr=1e-3, dr=20, qp=22, epoch=100, batchSize=200, predID=0,
                lambq=1.0, lambb0=0.8, lambb1=1.0, lambb2=1.2, lambd0=1.0, lambd1=1.0, lambd2=1.0, lambresb0=0.5, lambresb1=0.5, lambresb2=0.5,
                saveEvery=10, seed=0, resume=False, maxSteps=None, modelDir=None, valPrecision="f16x3", device=0)
    assert {k: getattr(a, k) for k in want} == want


@pytest.mark.parametrize("comp,qp,pred", [("Luma", 22, 0), ("Luma", 22, 1), ("Chroma", 27, 1)])
def test_plan_accepts_a_whole_directory(data, tmp_path, comp, qp, pred):
    p = plan(TC.argv(data, tmp_path, comp, pred, qp))
    assert p["comp"] == comp and sorted(p["sets"]) == sorted(TC.SETS) and all(s["n"] == 3 for s in p["sets"].values())
    assert (p["sets"]["Train"]["msbt"] is None) == (pred == 0)
    assert sorted(p["start"]) == (["Q"] if pred == 1 else [])


@pytest.mark.parametrize("flags,needle", [
    (dict(predID=3), "--predID"), (dict(qp=21), "--qp"), (dict(qp=42), "--qp"), (dict(lr=0), "--lr"), (dict(lr="nan"), "--lr"),
    (dict(dr=0), "--dr"), (dict(epoch=0), "--epoch"), (dict(batchSize=0), "--batchSize"), (dict(batchSize=65537), "--batchSize"),
    (dict(lambb1="inf"), "--lambb1"), (dict(saveEvery=0), "--saveEvery"), (dict(maxSteps=0), "--maxSteps"), (dict(seed=-1), "--seed"),
    (dict(device=-1), "--device"), (dict(valPrecision="fp16"), "--valPrecision"), (dict(jobID="a/b"), "--jobID"),
    (dict(modelDir="/nonexistent/models"), "--modelDir"), (dict(resume=True), "--resume"), (dict(predID=2), "--modelDir"),
])
def test_plan_refuses_each_bad_flag(data, tmp_path, capsys, flags, needle):
    f = dict(flags)
    pred = f.pop("predID", 0)
    refused(TC.argv(data, tmp_path, "Luma", pred, **f), capsys, needle)


def test_plan_refuses_a_missing_input_directory_and_missing_models(data, tmp_path, capsys):
    refused(TC.argv(tmp_path / "nowhere", tmp_path, "Luma", 0), capsys, "--inputDir")
    empty = tmp_path / "models"
    empty.mkdir()
    refused(TC.argv(data, tmp_path, "Luma", 2, modelDir=empty), capsys, "no weights for Luma_Q")
    refused(TC.argv(data, tmp_path, "Luma", 1, modelDir=empty), capsys, "no weights for Luma_Q")


def _copy(data, tmp_path):
    import shutil
    d = tmp_path / "copy"
    shutil.copytree(str(data), str(d))
    return d


@pytest.mark.parametrize("which", TC.SETS)
def test_plan_refuses_a_missing_file_of_each_set(data, tmp_path, capsys, which):
    d = _copy(data, tmp_path)
    os.remove(str(d / (which + "_Luma_QP22_MSBTdepth_Block16.npy")))
    refused(TC.argv(d, tmp_path, "Luma", 1), capsys, which + "_Luma_QP22_MSBTdepth_Block16.npy not found")
    plan(TC.argv(d, tmp_path, "Luma", 0))                           # --predID 0 does not read it
    os.remove(str(d / (which + "_Y_Block68.npy")))
    refused(TC.argv(d, tmp_path, "Luma", 0), capsys, which + "_Y_Block68.npy not found")


def test_plan_refuses_wrong_dtype_shape_and_count(data, tmp_path, capsys):
    d = _copy(data, tmp_path)
    name = str(d / "Validate_Luma_QP22_MSdirection_Block16.npy")
    good = np.load(name)
    np.save(name, good.astype(np.uint8))
    refused(TC.argv(d, tmp_path, "Luma", 2, modelDir=d), capsys, "expected int8[n,3,16,16]")
    np.save(name, good[:, :2])
    refused(TC.argv(d, tmp_path, "Luma", 1), capsys, "expected int8[n,3,16,16]")
    np.save(name, good[:2])
    refused(TC.argv(d, tmp_path, "Luma", 1), capsys, "2 labels for 3 QT label blocks")
    np.save(name, good)
    u = str(d / "TestSub_U_Block34.npy")
    np.save(u, np.load(u)[:1])
    refused(TC.argv(d, tmp_path, "Chroma", 0, 27), capsys, "1 blocks for 3 QT label blocks")


def test_plan_does_not_initialise_the_gpu(data, tmp_path):
    code = ("import sys; sys.path.insert(0, %r)\n"
            "from pmp_vvc_tip2023_amd import train_qbd as T\n"
            "T.plan(T.build_parser().parse_args(%r))\n"
            "import torch\n"
            "assert not torch.cuda.is_initialized()\n"
            "try:\n"
            "    T.plan(T.build_parser().parse_args(%r))\n"
            "except SystemExit as e:\n"
            "    assert e.code == 2 and not torch.cuda.is_initialized(); print('refused')\n") % (
                ROOT, TC.argv(data, tmp_path, "Luma", 1), TC.argv(data, tmp_path, "Luma", 1, qp=23))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "refused", r.stderr


def adjust_learning_rate(lr, optimizer, epoch, decay_rate):
    """Metrics.adjust_learning_rate (Metrics.py:53-57), its statements"""
    adj_lr = lr * (0.5 ** (epoch // decay_rate))
    if adj_lr > 1e-6:
        for param_group in optimizer.param_groups:
            param_group['lr'] = adj_lr


@pytest.mark.parametrize("lr,dr", [(1e-3, 20), (5e-4, 30), (2e-4, 7), (1e-6, 5)])
def test_learning_rate_rule_equals_the_references(lr, dr):
    class Opt:
        param_groups = [{"lr": lr}]
    opt, cur, held = Opt(), lr, 0
    for epoch in range(201):
        adjust_learning_rate(lr, opt, epoch, dr)
        new = T.learning_rate(lr, epoch, dr, cur)
        assert new == opt.param_groups[0]["lr"]
        held += lr * 0.5 ** (epoch // dr) <= 1e-6 and new == cur
        cur = new
    assert held > 0 or lr * 0.5 ** (200 // dr) > 1e-6        # where the floor is reached, the old value was held


def test_an_epochs_order_depends_on_seed_and_epoch_alone():
    from pmp_vvc_tip2023_amd import dataset as D
    a = D.permutation(12, True, 3, 1)
    D.permutation(12, True, 9, 0)
    assert a.tolist() == D.permutation(12, True, 3, 1).tolist() and sorted(a.tolist()) == list(range(12))
    assert a.tolist() != D.permutation(12, True, 3, 2).tolist() and a.tolist() != D.permutation(12, True, 4, 1).tolist()
    assert D.permutation(5, False, 3, 1).tolist() == [0, 1, 2, 3, 4]


def test_the_oracles_modules_learn_twice_the_margin_the_gpu_test_asserts(tmp_path):
    """The condition on the inputs of test_gpu_train_qbd's learning test: the same 30 steps on oracle/nets_torch.py's modules under
    torch.optim.Adam on the CPU drop from a mean of 51.930094 over the first 5 steps to 51.104221 over the last 5."""
    import torch
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    L = TC.LEARN
    sets = TC.write_sets(str(tmp_path), L["comp"], L["qp"], n=L["n"], sets=("Train",))
    losses = TC.oracle_learning(sets, L["comp"], L["seed"], L["steps"])
    first, last = float(np.mean(losses[:5])), float(np.mean(losses[-5:]))
    print("oracle: first 5 steps %.6f, last 5 steps %.6f" % (first, last))
    assert first - last >= 2 * L["margin"]
