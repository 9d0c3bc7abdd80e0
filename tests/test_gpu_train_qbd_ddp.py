"""GPU: python -m pmp_vvc_tip2023_amd.train_qbd --gpus N, whole runs.  Nothing here has a tolerance: a run on W ranks writes the bytes
of the one-rank run whose micro-batches are the ranks' slices.

Data as test_gpu_train_qbd.py's: Chroma at QP 27, 12 blocks per set, --predID 2 --batchSize 5 --epoch 2 --saveEvery 1 --seed 1, the
starting pair the shipped QT weights and synth.synth_msbd_weights.  Every job is a fresh child process (its ranks are its children)
in a session of its own under a time limit; a job that fails or runs out of time fails the test at once, its whole process group is
ended, and nothing is tried again.  The ranks share GPU 0 through the gloo backend (PMP_DIST_BACKEND=gloo, one visible device), at
most three at once.  The last test runs ONE rank with PMP_DIST_FORCE=1 on the RCCL backend, so that the RCCL gather itself runs.
Compared: every .pkl and .pmpw file and loss.txt byte for byte, and every tensor of last.pt (nets and optimiser state) bit for bit.
What none of this measures is the speed-up: that needs a node with several GPUs."""
import glob
import os
import signal
import subprocess
import sys

import numpy as np
import pytest
import torch

import train_qbd_cases as TC
from conftest import ROOT

pytestmark = pytest.mark.gpu
COMP, QP = "Chroma", 27
JOB_TIMEOUT_S = 300
RUN = dict(batchSize=5, epoch=2, saveEvery=1, seed=1)


@pytest.fixture(scope="module")
def data(tmp_path_factory):
    from pmp_vvc_tip2023_amd import synth, weights as W
    d, m = tmp_path_factory.mktemp("sets"), tmp_path_factory.mktemp("models")
    TC.write_sets(str(d), COMP, QP)
    W.save_pmpw(str(m / ("%s_Q_%d.pmpw" % (COMP, QP))), COMP + "_Q", QP, W.load_net_weights(COMP + "_Q", QP)[0])
    W.save_pmpw(str(m / ("%s_BD_%d.pmpw" % (COMP, QP))), COMP + "_MSBD", QP, synth.synth_msbd_weights(COMP, QP))
    return d, m


def job(data, out, env=None, **flags):
    """One run of the command in a child process of its own session -> its job directory.  Fails the test on a non-zero exit status
    or at the time limit (the session's processes are then ended)."""
    d, m = data
    e = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""), PMP_DIST_BACKEND="gloo", HIP_VISIBLE_DEVICES="0")
    for k, v in (env or {}).items():
        if v is None:
            e.pop(k, None)
        else:
            e[k] = v
    cmd = [sys.executable, "-m", "pmp_vvc_tip2023_amd.train_qbd"] + TC.argv(d, out, COMP, 2, QP, modelDir=m, **flags)
    p = subprocess.Popen(cmd, env=e, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, start_new_session=True)
    try:
        text, _ = p.communicate(timeout=JOB_TIMEOUT_S)
    except subprocess.TimeoutExpired:
        os.killpg(p.pid, signal.SIGKILL)
        p.communicate()
        pytest.fail("train_qbd %s did not end within %d s" % (flags, JOB_TIMEOUT_S))
    assert p.returncode == 0, "train_qbd %s ended with status %d:\n%s" % (flags, p.returncode, text[-3000:])
    return os.path.join(str(out), "0000"), text


def flat_tensors(obj, prefix=""):
    """{path: numpy array or plain value} of everything in a last.pt"""
    if isinstance(obj, dict):
        out = {}
        for k, v in obj.items():
            out.update(flat_tensors(v, "%s/%s" % (prefix, k)))
        return out
    if isinstance(obj, (list, tuple)):
        out = {}
        for i, v in enumerate(obj):
            out.update(flat_tensors(v, "%s/%d" % (prefix, i)))
        return out
    return {prefix: obj.numpy() if isinstance(obj, torch.Tensor) else obj}


def snapshot(job_dir):
    """{name: bytes} of the checkpoints, the .pmpw files and loss.txt, and {path: value} of last.pt"""
    names = sorted(glob.glob(os.path.join(job_dir, "*.pkl")) + glob.glob(os.path.join(job_dir, "*.pmpw")) + [os.path.join(job_dir, "loss.txt")])
    last = torch.load(os.path.join(job_dir, "last.pt"), map_location="cpu", weights_only=True)
    return {os.path.basename(p): open(p, "rb").read() for p in names}, flat_tensors(last)


def assert_same_run(got, want, what):
    (files, last), (wfiles, wlast) = got, want
    assert sorted(files) == sorted(wfiles), (what, sorted(files), sorted(wfiles))
    assert len([k for k in files if k.endswith(".pkl")]) == 4 and len([k for k in files if k.endswith(".pmpw")]) == 2 and "loss.txt" in files
    for k in wfiles:
        assert files[k] == wfiles[k], (what, k)
    assert sorted(last) == sorted(wlast) and any(k.startswith("/optim/state/") for k in last), what
    for k, v in wlast.items():
        if isinstance(v, np.ndarray):
            assert last[k].dtype == v.dtype and last[k].shape == v.shape and last[k].tobytes() == v.tobytes(), (what, k)
        else:
            assert last[k] == v, (what, k)


@pytest.fixture(scope="module")
def micro3(data, tmp_path_factory):
    """The one-rank run with --microBatch 3: what two ranks must write"""
    return snapshot(job(data, tmp_path_factory.mktemp("micro3"), microBatch=3, **RUN)[0])


@pytest.fixture(scope="module")
def two_ranks(data, tmp_path_factory):
    d, text = job(data, tmp_path_factory.mktemp("gpus2"), gpus=2, **RUN)
    return snapshot(d), text


def test_two_ranks_write_the_bytes_of_one_rank_with_micro_batches_of_3(micro3, two_ranks):
    """Batches of 5, 5 and 2 rows: rank 1 takes rows 3..4 of the full ones and none of the ragged last one."""
    snap, text = two_ranks
    assert_same_run(snap, micro3, "--gpus 2 against --microBatch 3")
    assert text.count("Start Training ...") == 1 and text.count("Epoch: 1 ") == 1, "rank 0 alone prints"


def test_three_ranks_write_the_bytes_of_one_rank_with_micro_batches_of_2(data, tmp_path):
    """Three sources: the order of the sum matters.  The ragged batch of 2 leaves ranks 1 and 2 empty."""
    one = snapshot(job(data, tmp_path / "micro2", microBatch=2, **RUN)[0])
    three = snapshot(job(data, tmp_path / "gpus3", gpus=3, **RUN)[0])
    assert_same_run(three, one, "--gpus 3 against --microBatch 2")


def test_two_ranks_resumed_write_the_bytes_of_the_whole_run(data, tmp_path, two_ranks):
    kw = dict(RUN, epoch=1)
    job(data, tmp_path, gpus=2, **kw)
    d, _ = job(data, tmp_path, gpus=2, resume=True, **RUN)
    assert_same_run(snapshot(d), two_ranks[0], "--gpus 2 --epoch 1, then --resume to epoch 2")


def test_one_forced_rank_on_rccl_writes_the_one_rank_bytes(data, tmp_path, micro3):
    """PMP_DIST_FORCE=1: a one-rank process group on the RCCL backend, so pack, all_gather_into_tensor and the sum of one bucket run"""
    d, text = job(data, tmp_path, env={"PMP_DIST_FORCE": "1", "PMP_DIST_BACKEND": None}, microBatch=3, **RUN)
    assert_same_run(snapshot(d), micro3, "one rank with a forced RCCL group against one rank without a group")
