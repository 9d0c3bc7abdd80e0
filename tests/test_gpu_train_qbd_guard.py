"""GPU: python -m pmp_vvc_tip2023_amd.train_qbd with the divergence guard (--clipNorm, --skipNonFinite, --maxSkipped), whole runs.
Nothing here has a tolerance but D's mean.

Data: Chroma at QP 27, 32 blocks per set of train_qbd_cases' synthetic sets, --predID 2 --batchSize 4 --maxSteps 8 --epoch 2
--saveEvery 1 --seed 1: 8 steps an epoch.  The starting pair is the shipped QT weights and synth.synth_msbd_weights.
  A  the guard with nothing to guard (--clipNorm 1e30 --skipNonFinite) writes the bytes of the run without it
  B  --clipNorm at a quarter of the largest norm A recorded (read from A's guard.txt) clips, ends well, and trains other parameters
  C  divergence: a good epoch at the default --lr, then --resume with --lr 1e30 --skipNonFinite --maxSkipped 3.  The first step of
     that epoch is taken (its gradients are finite) and moves every parameter by about 1e30; from the second forward pass on
     products of such parameters overflow float32, every gradient is NaN or inf and every step is skipped: status 5 before
     anything of the epoch is written.  1e30 does that on the device; no smaller rate was looked for
  D  one NaN planted in one gradient at step 3 of 8 (guard_plant): that step is skipped and the epoch's means are those of the
     other seven, computed here from the values Trainer.accumulate returned (within three float64 roundings: the test says which)
  E  the same plant on rank 1 of 2 ranks sharing the GPU over gloo: both ranks skip, and the files, guard.txt included, are the
     bytes of the one-rank run with --microBatch 2 and the plant in the whole batch's gradient
The in-process runs go through train_qbd.main; E's jobs are child processes in sessions of their own under a time limit, as
test_gpu_train_qbd_ddp.py's."""
import glob
import os
import signal
import subprocess
import sys

import numpy as np
import pytest
import torch

import guard_plant
import train_qbd_cases as TC
from conftest import ROOT
from test_gpu_train_qbd_ddp import assert_same_run, flat_tensors

pytestmark = pytest.mark.gpu
COMP, QP = "Chroma", 27
RUN = dict(batchSize=4, maxSteps=8, epoch=2, saveEvery=1, seed=1)
GUARD = dict(clipNorm=1e30, skipNonFinite=True)
JOB_TIMEOUT_S = 300


@pytest.fixture(scope="module")
def data(tmp_path_factory):
    from pmp_vvc_tip2023_amd import synth, weights as W
    d, m = tmp_path_factory.mktemp("sets"), tmp_path_factory.mktemp("models")
    TC.write_sets(str(d), COMP, QP, n=32)
    W.save_pmpw(str(m / ("%s_Q_%d.pmpw" % (COMP, QP))), COMP + "_Q", QP, W.load_net_weights(COMP + "_Q", QP)[0])
    W.save_pmpw(str(m / ("%s_BD_%d.pmpw" % (COMP, QP))), COMP + "_MSBD", QP, synth.synth_msbd_weights(COMP, QP))
    return d, m


def run(data, out, **flags):
    """train_qbd.main in this process -> (exit status, job directory)"""
    from pmp_vvc_tip2023_amd import train_qbd
    d, m = data
    return train_qbd.main(TC.argv(d, out, COMP, 2, QP, modelDir=m, **flags)), os.path.join(str(out), "0000")


def snapshot(job_dir, guard=True):
    names = sorted(glob.glob(os.path.join(job_dir, "*.pkl")) + glob.glob(os.path.join(job_dir, "*.pmpw")) + [os.path.join(job_dir, "loss.txt")] +
                   ([os.path.join(job_dir, "guard.txt")] if guard else []))
    last = torch.load(os.path.join(job_dir, "last.pt"), map_location="cpu", weights_only=True)
    return {os.path.basename(p): open(p, "rb").read() for p in names}, flat_tensors(last)


def guard_lines(job_dir):
    """guard.txt -> [(epoch, steps, skipped, clipped, max_run, max_norm)]"""
    rows = [ln.split(",") for ln in open(os.path.join(job_dir, "guard.txt")).read().split("\n") if ln]
    assert all(len(r) == 6 for r in rows)
    return [tuple(int(v) for v in r[:5]) + (float(r[5]),) for r in rows]


@pytest.fixture(scope="module")
def plain(data, tmp_path_factory):
    rc, job = run(data, tmp_path_factory.mktemp("plain"), **RUN)
    assert rc == 0 and not os.path.exists(os.path.join(job, "guard.txt"))
    return snapshot(job, guard=False)


@pytest.fixture(scope="module")
def guarded(data, tmp_path_factory):
    rc, job = run(data, tmp_path_factory.mktemp("guarded"), **RUN, **GUARD)
    assert rc == 0
    return job


def test_a_guard_with_nothing_to_guard_writes_the_unguarded_bytes(plain, guarded):
    files, last = snapshot(guarded)
    lines = guard_lines(guarded)
    assert [ln[:5] for ln in lines] == [(0, 8, 0, 0, 0), (1, 16, 0, 0, 0)] and 0 < lines[0][5] <= lines[1][5] < float("inf")
    files.pop("guard.txt")
    assert sorted(k for k in last if k.startswith("/guard/")) == ["/guard/" + k for k in sorted(("steps", "skipped", "clipped", "run", "max_run", "max_norm"))]
    assert last["/guard/steps"] == 16 and last["/guard/max_norm"] == lines[1][5]
    last = {k: v for k, v in last.items() if not k.startswith("/guard/")}
    assert_same_run((files, last), plain, "--clipNorm 1e30 --skipNonFinite against no flags")


def test_b_a_quarter_of_the_recorded_norm_clips_and_trains_other_parameters(data, tmp_path, guarded):
    max_norm = guard_lines(guarded)[-1][5]
    rc, job = run(data, tmp_path, **RUN, clipNorm=repr(max_norm / 4), skipNonFinite=True)
    assert rc == 0
    lines = guard_lines(job)
    assert lines[-1][1] == 16 and lines[-1][2] == 0 and lines[-1][3] > 0, lines
    a, b = snapshot(guarded)[0], snapshot(job)[0]
    pm = [k for k in a if k.endswith(".pmpw")]
    assert len(pm) == 2 and all(a[k] != b[k] for k in pm)
    assert all(np.isfinite(v).all() for k, v in snapshot(job)[1].items() if isinstance(v, np.ndarray))


def test_c_divergence_ends_with_status_5_and_keeps_the_last_good_epochs_files(data, tmp_path, capsys):
    from pmp_vvc_tip2023_amd import train_qbd
    rc, job = run(data, tmp_path, **dict(RUN, epoch=1))
    assert rc == 0
    keep = {os.path.basename(p): open(p, "rb").read() for p in glob.glob(os.path.join(job, "*"))}
    assert len([k for k in keep if k.endswith(".pmpw")]) == 2 and "last.pt" in keep and "guard.txt" not in keep
    capsys.readouterr()
    rc, _ = run(data, tmp_path, **RUN, resume=True, lr=1e30, skipNonFinite=True, maxSkipped=3)
    err = capsys.readouterr().err
    assert rc == train_qbd.EXIT_DIVERGED == 5, err[-2000:]
    assert "diverged in epoch 1" in err and "steps 8" in err and "skipped 7" in err and "max_run 7" in err and "--maxSkipped 3" in err, err[-2000:]
    after = {os.path.basename(p): open(p, "rb").read() for p in glob.glob(os.path.join(job, "*"))}
    assert after == keep, "the bad epoch wrote or changed %s" % sorted(k for k in after if after[k] != keep.get(k))


def test_d_one_planted_nan_skips_one_step_and_the_means_are_the_other_sevens(data, tmp_path, monkeypatch):
    kept = []
    guard_plant.plant(monkeypatch.setattr, 3, None, kept)
    rc, job = run(data, tmp_path, **dict(RUN, epoch=1), skipNonFinite=True)
    assert rc == 0 and len(kept) == 8
    assert guard_lines(job) == [(0, 8, 1, 0, 1, guard_lines(job)[0][5])]
    files, last = snapshot(job)
    assert all(np.isfinite(v).all() for k, v in last.items() if isinstance(v, np.ndarray) and (k.startswith("/nets/") or k.startswith("/optim/state/")))
    assert all(last["/optim/state/%d/step" % i] == 8.0 for i in range(92)), "the skipped step counted"
    values = torch.stack(kept).cpu().numpy()
    assert values.dtype == np.float64 and np.isfinite(values).all()
    total = np.zeros(values.shape[1])
    for i in (0, 1, 3, 4, 5, 6, 7):                                   # in step order, as the device adds them
        total = total + values[i]
    mean = total / 7
    got = np.array([float(v) for v in files["loss.txt"].decode().split("\n")[1].split(",")[:-1]])
    # the same float64 sum in the same order, then a division by 7.  The run divides a device tensor by a Python number, which torch
    # may compute as a product with the rounded reciprocal: 1/7 rounded, the product rounded, and this quotient rounded are three
    # roundings of relative size 2^-53 at most.  Leaving the skipped step in, or dividing by 8, is off by parts in a hundred
    assert got.shape == mean.shape == (8,)
    assert (np.abs(got - mean) <= 3 * 2.0 ** -53 * np.abs(mean)).all(), (got.tolist(), mean.tolist())
    assert abs(got[0] - values[:, 0].mean()) > 1e-6 * got[0] and abs(got[0] - (total[0] + values[2, 0]) / 8) > 1e-6 * got[0]


def job(data, out, step, rank, **flags):
    """tests/guard_plant.py STEP RANK with train_qbd's arguments, as a child process of its own session -> its job directory"""
    d, m = data
    e = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""), PMP_DIST_BACKEND="gloo", HIP_VISIBLE_DEVICES="0")
    cmd = [sys.executable, os.path.join(ROOT, "tests", "guard_plant.py"), str(step), str(rank)] + TC.argv(d, out, COMP, 2, QP, modelDir=m, **flags)
    p = subprocess.Popen(cmd, env=e, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, start_new_session=True)
    try:
        text, _ = p.communicate(timeout=JOB_TIMEOUT_S)
    except subprocess.TimeoutExpired:
        os.killpg(p.pid, signal.SIGKILL)
        p.communicate()
        pytest.fail("train_qbd %s did not end within %d s" % (flags, JOB_TIMEOUT_S))
    assert p.returncode == 0, "train_qbd %s ended with status %d:\n%s" % (flags, p.returncode, text[-3000:])
    return os.path.join(str(out), "0000")


def test_e_two_ranks_skip_together_and_write_the_one_rank_bytes(data, tmp_path):
    one = job(data, tmp_path / "micro2", 3, -1, microBatch=2, **RUN, **GUARD)
    two = job(data, tmp_path / "gpus2", 3, 1, gpus=2, **RUN, **GUARD)
    assert [ln[:5] for ln in guard_lines(one)] == [(0, 8, 1, 0, 1), (1, 16, 1, 0, 1)]
    a, b = snapshot(two), snapshot(one)
    assert "guard.txt" in a[0] and a[0]["guard.txt"] == b[0]["guard.txt"]
    without = lambda s: ({k: v for k, v in s[0].items() if k != "guard.txt"}, s[1])
    assert_same_run(without(a), without(b), "--gpus 2 against --microBatch 2, one NaN planted at step 3")
