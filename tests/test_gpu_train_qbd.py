"""GPU: python -m pmp_vvc_tip2023_amd.train_qbd, through its main().

Data: 12 blocks per set (Train, Validate, TestSub) of synth.recipe_r_blocks pixels and val_cases' seeded labels under the reference's
file names (train_qbd_cases.write_sets); Luma at QP 22 and Chroma at QP 27.  --batchSize 5 leaves a ragged last batch of 2.
--predID 2 starts from the shipped QT weights and synth.synth_msbd_weights, saved as the --modelDir pair.
The micro-batch test compares the QT net's .grad of one step of 300 rows (256 + 44) with the gradient of the same loss through
oracle.nets_torch.q_forward in float64 on the CPU: every parameter's gradient within 4 * d32 in the relative max norm, d32 the same
computation's float32 distance from float64 (test_gpu_q_net.py's yardstick).  As the 300 rows repeat 12 blocks, the float64 loss is
the sum over the 12 blocks of (rows that name the block / 300) * the block's mean L1.
Learning (train_qbd_cases.LEARN): Chroma --predID 0 --seed 1, 8 blocks as one batch, 30 steps at the default lr: the mean loss of the
last 5 steps lies at least 0.4 below the mean of the first 5.  The same steps on the oracle's modules under torch's Adam on the CPU go
from a mean of 51.930094 to 51.104221, a drop of 0.826, twice the margin (test_train_qbd_cpu.py asserts that): a condition on the
inputs, not a tolerance taken from the code under test."""
import glob
import os
import re

import numpy as np
import pytest
import torch

import conftest  # noqa: F401 - puts tools/ on sys.path
import train_qbd_cases as TC
import train_rig as R
from oracle import nets_torch as O

pytestmark = pytest.mark.gpu
eng = R.engine_fixture()
NETS = {"Luma": 22, "Chroma": 27}
FLOAT = r"-?\d+\.\d{6}"


@pytest.fixture(scope="module")
def data(tmp_path_factory):
    """-> (directory of both components' sets, their arrays, a --modelDir with the starting pair of each component)"""
    from pmp_vvc_tip2023_amd import synth, weights as W
    d, m = tmp_path_factory.mktemp("sets"), tmp_path_factory.mktemp("models")
    arrays = {comp: TC.write_sets(str(d), comp, qp) for comp, qp in NETS.items()}
    for comp, qp in NETS.items():
        W.save_pmpw(str(m / ("%s_Q_%d.pmpw" % (comp, qp))), comp + "_Q", qp, W.load_net_weights(comp + "_Q", qp)[0])
        W.save_pmpw(str(m / ("%s_BD_%d.pmpw" % (comp, qp))), comp + "_MSBD", qp, synth.synth_msbd_weights(comp, qp))
    return d, arrays, m


def run(data, out, comp, pred, **flags):
    from pmp_vvc_tip2023_amd import train_qbd
    d, _, m = data
    if pred == 2:
        flags.setdefault("modelDir", m)
    assert train_qbd.main(TC.argv(d, out, comp, pred, NETS[comp], **flags)) == 0
    return os.path.join(str(out), "0000")


def files(job, pattern):
    return sorted(glob.glob(os.path.join(job, pattern)))


@pytest.mark.parametrize("comp", list(NETS))
@pytest.mark.parametrize("pred", [0, 1, 2])
def test_all_three_modes_write_the_references_files_and_a_pair_that_validates_to_the_printed_numbers(data, tmp_path, capsys, pred, comp):
    from pmp_vvc_tip2023_amd import engine as E, train_qbd, weights as W
    qp = NETS[comp]
    job = run(data, tmp_path, comp, pred, batchSize=5, epoch=2, saveEvery=1)
    printed = capsys.readouterr().out
    # loss.txt: the reference's header, one line of the right column count per epoch, finite numbers
    lines = open(os.path.join(job, "loss.txt")).read().split("\n")
    assert lines[0] + "\n" == train_qbd.HEADERS[pred] and lines[3:] == [""]
    rows = []
    for ln in lines[1:3]:
        assert ln.endswith(",")
        rows.append([float(v) for v in ln[:-1].split(",")])
        assert len(rows[-1]) == train_qbd.COLUMNS[pred] and np.isfinite(rows[-1]).all()
    # checkpoints under the reference's names, plain state_dicts
    kinds = {0: ("Q",), 1: ("BD",), 2: ("Q", "BD")}[pred]
    nfloat = 4 if pred == 2 else 3
    for kind in kinds:
        for epoch in (0, 1):
            got = files(job, "%s_%s_%d_epoch_%d_*.pkl" % (comp, kind, qp, epoch))
            assert len(got) == 1 and re.fullmatch(r"%s_%s_%d_epoch_%d(_-?\d+\.\d{4}){%d}\.pkl" % (comp, kind, qp, epoch, nfloat), os.path.basename(got[0])), got
            sd = W.load_pkl(got[0])
            assert len(sd) == (20 if kind == "Q" else 72) and all(v.dtype == np.float32 and np.isfinite(v).all() for v in sd.values())
    assert len(files(job, "*.pkl")) == 2 * len(kinds) and os.path.isfile(os.path.join(job, "last.pt"))
    last = W.load_pkl(files(job, "%s_%s_%d_epoch_1_*.pkl" % (comp, kinds[-1], qp))[0])
    man, pm = W.load_pmpw(os.path.join(job, "%s_%s_%d.pmpw" % (comp, kinds[-1], qp)))
    assert sorted(pm) == sorted(last) and all(R.same_bits(pm[k], last[k]) for k in pm), "the .pmpw holds the latest epoch"
    # the pair in a fresh engine gives the numbers the run printed for its last epoch
    sets = data[1][comp]
    fresh = E.Engine(0, weight_dir=job, allow_synthetic_mtt=pred == 0)
    try:
        res = []
        for name in ("Validate", "TestSub"):
            s = sets[name]
            blocks = s["y"] if comp == "Luma" else (s["y"], s["u"], s["v"])
            if pred == 2:
                res.append(fresh.validation_QBD(comp, qp, blocks, s["qt8"], s["msbt"], s["msdire"], batch_size=5))
            else:
                res.append(fresh.pre_validation(comp, qp, pred, blocks, s["qt8"], s["msbt"], s["msdire"], batch_size=5))
    finally:
        fresh.close()
    epoch1 = printed[printed.index("Epoch: 1 "):]
    if pred == 0:
        assert rows[1][3:] == [res[0][0], res[0][1], res[1][0], res[1][1]], "loss.txt holds the validation numbers in full"
        assert "Val: Loss: %.6f  Acc: %.6f\n" % tuple(res[0]) in epoch1 and "Test: Loss: %.6f  Acc: %.6f\n" % tuple(res[1]) in epoch1
    else:
        nl1 = 6 if pred == 1 else 7
        fmt = ("[B] %.6f %.6f %.6f [D] %.6f %.6f %.6f" if pred == 1 else "[Q] %.6f [B] %.6f %.6f %.6f [D] %.6f %.6f %.6f") + "\n"
        for what, r in zip(("Val", "Test"), res):
            assert ("%s L1: " % what) + fmt % tuple(r[:nl1]) in epoch1 and ("%s Accu: " % what) + fmt % tuple(r[nl1:2 * nl1]) in epoch1
        assert re.search(r"Epoch: 1  Loss: %s %.6f %.6f\n" % (FLOAT, res[0][-1], res[1][-1]), epoch1)


def snapshot(job):
    """{file name: bytes} of the checkpoints and the .pmpw files of a job directory"""
    return {os.path.basename(p): open(p, "rb").read() for p in files(job, "*.pkl") + files(job, "*.pmpw")}


def test_one_seed_gives_the_same_bytes_a_resumed_run_too_and_another_seed_others(data, tmp_path):
    comp = "Chroma"
    kw = dict(batchSize=5, saveEvery=1)
    whole = snapshot(run(data, tmp_path / "a", comp, 2, seed=1, epoch=2, **kw))
    assert len(whole) == 6
    assert snapshot(run(data, tmp_path / "b", comp, 2, seed=1, epoch=2, **kw)) == whole, "two runs with one seed"
    first = snapshot(run(data, tmp_path / "c", comp, 2, seed=1, epoch=1, **kw))
    assert len(first) == 4 and all(whole[k] == v for k, v in first.items() if k.endswith(".pkl"))
    assert snapshot(run(data, tmp_path / "c", comp, 2, seed=1, epoch=2, resume=True, **kw)) == whole, "one epoch, then --resume for the second"
    assert open(os.path.join(str(tmp_path / "c"), "0000", "loss.txt")).read() == open(os.path.join(str(tmp_path / "a"), "0000", "loss.txt")).read()
    other = snapshot(run(data, tmp_path / "d", comp, 2, seed=2, epoch=1, **kw))
    pm = [k for k in first if k.endswith(".pmpw")]
    assert len(pm) == 2 and all(other[k] != first[k] for k in pm), "a different seed"


def q_weights(comp):
    from pmp_vvc_tip2023_amd import weights as W
    return {k: np.asarray(v, np.float32) for k, v in W.load_net_weights(comp + "_Q", NETS[comp])[0].items()}


def test_a_batch_of_300_runs_as_256_and_44_and_its_gradients_are_the_whole_batchs(eng, data):
    from pmp_vvc_tip2023_amd import dataset, train_qbd
    comp, qp = "Chroma", NETS["Chroma"]
    d, arrays, _ = data
    args = train_qbd.build_parser().parse_args(TC.argv(d, "/nonexistent", comp, 0, qp, batchSize=300))
    index = torch.from_numpy(np.random.default_rng(4).integers(0, 12, 300).astype(np.int64))
    try:
        trainer = train_qbd.Trainer(eng, args, comp, {}, 0)
        trainer.nets["Q"].load_state_dict({k: torch.from_numpy(v) for k, v in q_weights(comp).items()})
        train = dataset.DeviceDataset(eng, str(d), comp, qp, "Train", 0, 0)
        batch = train.gather(index.cuda(), 300)
        sizes, inner = [], trainer.forward_loss
        trainer.forward_loss = lambda part: (sizes.append(part[0].shape[0]), inner(part))[1]
        values = trainer.accumulate(batch)
        torch.cuda.synchronize()
        train.check()
    finally:
        eng.set_stream(0)
    assert sizes == [256, 44]
    # float64 and float32 on the CPU: the 12 blocks, each weighted by the rows that name it
    torch.set_num_threads(16)
    s = arrays[comp]["Train"]
    x = O.chroma_input(s["y"], s["u"], s["v"])
    ql = torch.from_numpy((s["qt8"] - np.uint8(1)).astype(np.float64))[:, None]
    share = torch.from_numpy(np.bincount(index.numpy(), minlength=12) / 300.0)
    grads, loss = {}, {}
    for dt in (torch.float64, torch.float32):
        w = {k: torch.from_numpy(v).to(dt).requires_grad_() for k, v in q_weights(comp).items()}
        per_block = (O.q_forward(w, x.to(dt), False) - ql.to(dt)).abs().mean(dim=(1, 2, 3))
        total = (per_block * share.to(dt)).sum()
        total.backward()
        loss[dt] = total.detach()
        grads[dt] = {k: v.grad.double().numpy() for k, v in w.items()}
    g64, g32 = grads[torch.float64], grads[torch.float32]
    dist = lambda a, b: float(np.abs(a - b).max() / np.abs(b).max())
    d32 = max(dist(g32[k], g64[k]) for k in g64)
    params = dict(trainer.nets["Q"].named_parameters())
    worst = {k: dist(params[k].grad.cpu().double().numpy(), g64[k]) for k in g64}
    print("d32 %.3g; largest distance %.3g (%.2f d32); loss %.9g against %.9g in float64" %
          (d32, max(worst.values()), max(worst.values()) / d32, float(values[0]), float(loss[torch.float64])))
    assert sorted(params) == sorted(g64) and all(np.abs(v).max() > 0 for v in g64.values())
    for k, v in worst.items():
        assert v <= 4 * d32, (k, v, d32)
    assert abs(float(values[0]) - float(loss[torch.float64])) <= 4 * abs(float(loss[torch.float32]) - float(loss[torch.float64])) + 1e-6 * float(loss[torch.float64])
    assert abs(float(values[1]) - float(values[0])) <= 1e-6 * float(values[0]), "pre_train_Q's L1 loss is its loss"


def test_thirty_steps_on_one_batch_learn(eng, tmp_path):
    from pmp_vvc_tip2023_amd import dataset, train_qbd
    L = TC.LEARN
    TC.write_sets(str(tmp_path), L["comp"], L["qp"], n=L["n"], sets=("Train",))
    args = train_qbd.build_parser().parse_args(TC.argv(tmp_path, "/nonexistent", L["comp"], 0, L["qp"], batchSize=L["n"], seed=L["seed"]))
    assert args.lr == 1e-3
    try:
        trainer = train_qbd.Trainer(eng, args, L["comp"], {}, 0)
        start = TC.initial_q_weights(False, L["seed"])
        assert all(R.same_bits(R.num(v), start[k].numpy()) for k, v in trainer.nets["Q"].state_dict().items()), "the oracle's run starts from the same net"
        train = dataset.DeviceDataset(eng, str(tmp_path), L["comp"], L["qp"], "Train", 0, 0)
        losses = []
        for step in range(L["steps"]):
            for batch in train.batches(L["n"], True, L["seed"], step):
                losses.append(trainer.step(batch)[0])
        losses = torch.stack(losses).tolist()
    finally:
        eng.set_stream(0)
    first, last = float(np.mean(losses[:5])), float(np.mean(losses[-5:]))
    print("first 5 steps %.6f, last 5 steps %.6f" % (first, last))
    assert len(losses) == 30 and np.isfinite(losses).all() and last < first - L["margin"]
