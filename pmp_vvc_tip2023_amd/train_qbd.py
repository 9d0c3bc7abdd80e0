"""Train_QBD.py's three training modes on this library, resident on the GPU.

    python -m pmp_vvc_tip2023_amd.train_qbd --predID 0|1|2 [--isLuma] --inputDir D --outDir O [--jobID 0000] [--lr 1e-3] [--dr 20]
           [--qp 22] [--epoch 100] [--batchSize 200] [--lambq .. --lambresb2 ..]
           [--modelDir M] [--seed 0] [--saveEvery 10] [--resume] [--maxSteps K] [--device 0] [--valPrecision f16x3|bf16x6|fp32]

--predID 0 is pre_train_Q (the QT net on the plain L1 loss, Train_QBD.py:117-191), 1 is pre_train_BD (the MTT net teacher-forced with
the QT labels on loss_func_MSBD, :193-303), 2 is train_QBD (both nets jointly on loss_func_QBD, starting from the pair <comp>_Q_<qp> and
<comp>_BD_<qp> (.pmpw or .pkl) in --modelDir, :305-429).  The reference's flags keep their names and defaults.  --inputDir holds the
three sets Train, Validate and TestSub in the reference's file names (validate.py's docstring); results go to <outDir>/<jobID>/.

A step: the learning rate by Metrics.adjust_learning_rate's rule, a batch gathered on the device (dataset.DeviceDataset), the nets'
forward (q_net.QNet, msbd_net.MSBDNet), the loss (train_loss), backward(), optim.Adam.step() - one launch.  A batch of more than 256
blocks, which the training calls do not take, runs as micro-batches of at most 256 whose losses are weighted n_i / n and whose
gradients add up in .grad, so --batchSize 400 works.  The numbers the reference reads with .item() at every step come from the loss
call's thirteen sums and are added up on the device; the host reads them once per epoch and at step % 1000 == 0 for the progress line.

An epoch ends as the reference's: Engine.pre_validation / Engine.validation_QBD of the current parameters (loaded into the engine
with Engine.load_pretrain_model, on the --valPrecision datapath) on the Validate and TestSub sets, the reference's printed lines, and
one line of loss.txt under the reference's header: an epoch value is the mean of the step values.  Every --saveEvery epochs the
checkpoints are written under the reference's names (<comp>_Q_<qp>_epoch_%d_....pkl, <comp>_BD_...: plain state_dicts,
weights.load_pkl reads them), and at every epoch <comp>_Q_<qp>.pmpw / <comp>_BD_<qp>.pmpw of the nets as they are now - the directory
then serves as --modelDir of inference_qbd and validate - and last.pt (nets, optimiser, epoch, seed), from which --resume continues.
--predID 1 also writes the QT net it validated with as <comp>_Q_<qp>.pmpw, so that the pair is whole.

What differs from the reference: the order of the batches is defined by --seed (dataset.permutation of (seed, epoch): a resumed run
gives the bits of an uninterrupted one); no nn.DataParallel (one GPU, state_dict names without "module."); micro-batches; --predID 0
validates beside the MTT net found in --modelDir or else the synthetic one, whose logits are dropped.
Flags, the three sets' files and the model files are checked before anything touches the GPU: exit status 2 on the first problem.
"""
import argparse
import math
import os
import sys

LAMBS = ("lambq", "lambb0", "lambb1", "lambb2", "lambd0", "lambd1", "lambd2", "lambresb0", "lambresb1", "lambresb2")
SETS = ("Train", "Validate", "TestSub")
HEADERS = {0: "epoch_loss, epoch_loss, epoch_L1_loss, val_L1_loss, val_accu, test_L1_loss, test_accu\n",
           1: "epoch_loss, epoch_b0_L1_loss, epoch_b1_L1_loss, epoch_b2_L1_loss, val_b2_accu, test_b2_accu\n",
           2: "epoch_loss, epoch_b0_L1_loss, epoch_b1_L1_loss, epoch_b2_L1_loss, val_b2_accu, test_b2_accu\n"}
COLUMNS = {0: 7, 1: 7, 2: 8}            # values per line of loss.txt (the reference's headers name fewer)
MICRO = 256                             # the largest n the training calls take


def build_parser():
    p = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    p.add_argument("--jobID", type=str, default="0000")
    p.add_argument("--isLuma", dest="isLuma", action="store_true")
    p.add_argument("--inputDir", type=str, default="/input/")
    p.add_argument("--inputDir1", type=str, default="/input/", help="unused, as in the reference")
    p.add_argument("--outDir", type=str, default="/output/")
    p.add_argument("--lr", default=1e-3, type=float, help="learning rate")
    p.add_argument("--dr", default=20, type=int, help="decay rate of lr")
    p.add_argument("--qp", default=22, type=int, help="quantization step")
    p.add_argument("--epoch", default=100, type=int, help="number of total epoch")
    p.add_argument("--batchSize", default=200, type=int, help="batch size")
    for k in ("lamb0", "lamb1", "lamb2"):
        p.add_argument("--" + k, default=1.0, type=float, help="unused, as in the reference")
    p.add_argument("--predID", default=0, type=int, help="0 pre_train_Q, 1 pre_train_BD, 2 train_QBD")
    for k, v in zip(LAMBS, (1.0, 0.8, 1.0, 1.2, 1.0, 1.0, 1.0, 0.5, 0.5, 0.5)):
        p.add_argument("--" + k, default=v, type=float, help="weight of loss function")
    p.add_argument("--modelDir", default=None, help="--predID 2: the pretrained pair to start from; otherwise where the partner net is looked for")
    p.add_argument("--seed", default=0, type=int, help="batch order and, for --predID 0 and 1, the initial weights")
    p.add_argument("--saveEvery", default=10, type=int, help="epochs between checkpoints")
    p.add_argument("--resume", action="store_true", help="continue from <outDir>/<jobID>/last.pt")
    p.add_argument("--maxSteps", default=None, type=int, help="steps per epoch at most (tests)")
    p.add_argument("--device", default=0, type=int)
    p.add_argument("--valPrecision", default="f16x3", help="datapath of the validation passes: f16x3, bf16x6 or fp32")
    return p


def learning_rate(lr, epoch, decay_rate, current):
    """Metrics.adjust_learning_rate (Metrics.py:53-57): lr * 0.5 ** (epoch // decay_rate) if that is above 1e-6, else the current one."""
    adj = lr * (0.5 ** (epoch // decay_rate))
    return adj if adj > 1e-6 else current


def plan(args):
    """Checks every flag, opens the three sets (validate.read_set) and finds the model files -> {"comp", "sets": {name: read_set's
    dict}, "start": {net: (kind, path)} of --predID 2's pair, "out_dir"}.  SystemExit(2) on the first problem, nothing has touched the GPU."""
    from . import weights as W
    from .validate import read_set

    def fail(msg):
        print("train_qbd: " + msg, file=sys.stderr)
        raise SystemExit(2)
    if args.predID not in (0, 1, 2):
        fail("--predID must be 0, 1 or 2, got %r" % args.predID)
    if not 22 <= args.qp <= 41:
        fail("--qp must be in 22..41 (the rows of the reference's weight_mat), got %d" % args.qp)
    if not (math.isfinite(args.lr) and args.lr > 0):
        fail("--lr must be a positive number")
    if args.dr < 1:
        fail("--dr must be >= 1")
    if not 1 <= args.epoch < (1 << 20):
        fail("--epoch must be in 1 .. 2^20 - 1")
    if not 1 <= args.batchSize <= 65536:
        fail("--batchSize must be in 1 .. 65536")
    for k in LAMBS:
        if not math.isfinite(getattr(args, k)):
            fail("--%s must be finite" % k)
    if args.saveEvery < 1:
        fail("--saveEvery must be >= 1")
    if args.maxSteps is not None and args.maxSteps < 1:
        fail("--maxSteps must be >= 1")
    if args.seed < 0 or args.seed >= (1 << 40):
        fail("--seed must be in 0 .. 2^40 - 1")
    if args.device < 0:
        fail("--device must be >= 0")
    if args.valPrecision not in ("f16x3", "bf16x6", "fp32"):
        fail("--valPrecision must be f16x3, bf16x6 or fp32, got %r" % args.valPrecision)
    if not args.jobID or os.sep in args.jobID:
        fail("--jobID must be a plain name")
    if not os.path.isdir(args.inputDir):
        fail("--inputDir %s is not a directory" % args.inputDir)
    if args.modelDir is not None and not os.path.isdir(args.modelDir):
        fail("--modelDir %s is not a directory" % args.modelDir)
    if args.predID == 2 and args.modelDir is None:
        fail("--predID 2 starts from a pretrained pair: --modelDir is required")
    comp = "Luma" if args.isLuma else "Chroma"
    out = {"comp": comp, "out_dir": os.path.join(args.outDir, args.jobID), "start": {}}
    out["sets"] = {name: read_set(args.inputDir, name, comp, args.qp, args.predID != 0, fail) for name in SETS}
    need = {0: (), 1: ("Q",), 2: ("Q", "MSBD")}[args.predID]       # 1: the QT net the MTT net is validated beside
    for kind in need:
        try:
            out["start"][kind] = W.find_net_weights("%s_%s" % (comp, kind), args.qp, args.modelDir)
        except FileNotFoundError as e:
            fail(str(e))
    if args.resume and not os.path.isfile(os.path.join(out["out_dir"], "last.pt")):
        fail("--resume: %s not found" % os.path.join(out["out_dir"], "last.pt"))
    return out


def loss_dict(args):
    return {k: getattr(args, k) for k in LAMBS}


def read_weights(kind_path):
    from . import weights as W
    kind, path = kind_path
    return W.load_pmpw(path)[1] if kind == "pmpw" else W.load_pkl(path)


class Trainer:
    """The nets, the optimiser and the step of one mode.  step_values: the numbers the reference appends to its lists at every step,
    [loss, the mode's L1 losses], a float64 device tensor."""
    NAMES = {0: ("Q",), 1: ("MSBD",), 2: ("Q", "MSBD")}

    def __init__(self, engine, args, comp, start, device):
        """start: plan()'s {net kind: (file kind, path)} of --predID 2's pair; empty: torch's initialisation there too (timing tools)"""
        import torch

        from . import msbd_net, optim, q_net
        self.engine, self.args, self.comp, self.luma = engine, args, comp, comp == "Luma"
        self.device = torch.device("cuda", int(device))
        torch.manual_seed(args.seed)                      # the initial weights of --predID 0 and 1
        self.nets = {}
        for kind in self.NAMES[args.predID]:
            net = q_net.QNet(engine, self.luma) if kind == "Q" else msbd_net.MSBDNet(engine, self.luma)
            if args.predID == 2 and start:
                net.load_state_dict({k: torch.from_numpy(v) for k, v in read_weights(start[kind]).items()})
            self.nets[kind] = net.to(self.device)
        self.optimizer = optim.Adam(engine, [p for net in self.nets.values() for p in net.parameters()], lr=args.lr)
        self.nvalues = {0: 2, 1: 7, 2: 8}[args.predID]

    def forward_loss(self, batch):
        """One micro-batch -> (loss, the step's L1 SUMS as the reference orders its L1 losses: float64 device tensor)"""
        from . import train_loss as TL
        a, e = self.args, self.engine
        if a.predID == 0:
            x, _, qt8 = batch
            loss, t = TL.l1_loss_Q(e, self.nets["Q"](x), qt8, return_terms=True)
            return loss, t[0:1] / 64.0
        x, qt_f, msbt, msdire, qt8 = batch
        if a.predID == 1:
            out = self.nets["MSBD"](x, qt_f)
            loss, t = TL.loss_func_MSBD(e, out[0], out[1], out[2], msbt, msdire, self.luma, a.qp, params=loss_dict(a), return_terms=True)
            return loss, t[1:7] / 256.0
        q = self.nets["Q"](x)
        out = self.nets["MSBD"](x, q)
        loss, t = TL.loss_func_QBD(e, q, out[0], out[1], out[2], qt8, msbt, msdire, self.luma, a.qp, params=loss_dict(a), return_terms=True)
        import torch
        return loss, torch.cat([t[0:1] / 64.0, t[1:7] / 256.0])

    def accumulate(self, batch):
        """zero_grad, then forward and backward of the batch in micro-batches of at most MICRO blocks -> step_values.  The .grads hold
        the gradient of the whole batch's loss."""
        import torch
        self.optimizer.zero_grad(set_to_none=True)
        n = batch[0].shape[0]
        values = torch.zeros(self.nvalues, dtype=torch.float64, device=self.device)
        for s in range(0, n, MICRO):
            part = tuple(t[s:s + MICRO] for t in batch)
            w = part[0].shape[0] / n
            loss, l1 = self.forward_loss(part)
            (loss * w if w != 1.0 else loss).backward()
            values[0] += loss.detach().double() * w
            values[1:] += l1 / n
        return values

    def step(self, batch):
        values = self.accumulate(batch)
        self.optimizer.step()
        return values

    def numpy_weights(self, kind):
        return {k: v.detach().cpu().numpy() for k, v in self.nets[kind].state_dict().items()}


def validate(engine, args, comp, sets, trainer, partner):
    """The epoch's validation: the current parameters into the engine, then pre_validation / validation_QBD on Validate and TestSub
    -> (val list, test list)."""
    for kind in trainer.nets:
        engine.load_pretrain_model("%s_%s" % (comp, kind), args.qp, trainer.numpy_weights(kind))
    for kind, w in partner.items():
        if not engine.has_weights("%s_%s" % (comp, kind), args.qp):
            engine.load_pretrain_model("%s_%s" % (comp, kind), args.qp, w)
    out = []
    for name in SETS[1:]:
        d = sets[name]
        if args.predID == 2:
            out.append(engine.validation_QBD(comp, args.qp, d["blocks"], d["qt8"], d["msbt"], d["msdire"], batch_size=args.batchSize))
        else:
            out.append(engine.pre_validation(comp, args.qp, args.predID, d["blocks"], d["qt8"], d["msbt"], d["msdire"], batch_size=args.batchSize))
    return out


def report(args, comp, epoch, mean, val, test):
    """The reference's printed lines of an epoch -> (the values of its loss.txt line, {net kind: checkpoint file name})"""
    bar = "*" * 130
    qp = str(args.qp)
    print(bar)
    if args.predID == 0:
        print("Epoch: %d  Loss: %.6f  L1 Loss %.6f" % (epoch, mean[0], mean[1]))
        print("Val: Loss: %.6f  Acc: %.6f" % (val[0], val[1]))
        print("Test: Loss: %.6f  Acc: %.6f" % (test[0], test[1]))
        line = [mean[0], mean[0], mean[1], val[0], val[1], test[0], test[1]]
        names = {"Q": comp + "_Q_" + qp + "_epoch_%d_%.4f_%.4f_%.4f.pkl" % (epoch, mean[0], val[0], test[0])}
    elif args.predID == 1:
        print("Epoch: %d  Loss: %.6f %.6f %.6f" % (epoch, mean[0], val[12], test[12]))
        print("Train L1: [B] %.6f %.6f %.6f [D] %.6f %.6f %.6f" % tuple(mean[1:7]))
        for what, v in (("Val", val), ("Test", test)):
            print("%s L1: [B] %.6f %.6f %.6f [D] %.6f %.6f %.6f" % ((what,) + tuple(v[0:6])))
            print("%s Accu: [B] %.6f %.6f %.6f [D] %.6f %.6f %.6f" % ((what,) + tuple(v[6:12])))
        line = list(mean[0:7])
        names = {"MSBD": comp + "_BD_" + qp + "_epoch_%d_%.4f_%.4f_%.4f.pkl" % (epoch, mean[0], val[12], test[12])}
    else:
        print("Epoch: %d  Loss: %.6f %.6f %.6f" % (epoch, mean[0], val[14], test[14]))
        print("Train L1: [Q] %.6f [B] %.6f %.6f %.6f [D] %.6f %.6f %.6f" % tuple(mean[1:8]))
        for what, v in (("Val", val), ("Test", test)):
            print("%s L1: [Q] %.6f [B] %.6f %.6f %.6f [D] %.6f %.6f %.6f" % ((what,) + tuple(v[0:7])))
            print("%s Accu: [Q] %.6f [B] %.6f %.6f %.6f [D] %.6f %.6f %.6f" % ((what,) + tuple(v[7:14])))
        line = list(mean[0:8])
        names = {"Q": comp + "_Q_" + qp + "_epoch_%d_%.4f_%.4f_%.4f_%.4f.pkl" % (epoch, mean[1], mean[0], val[12], test[12]),
                 "MSBD": comp + "_BD_" + qp + "_epoch_%d_%.4f_%.4f_%.4f_%.4f.pkl" % (epoch, mean[4], mean[0], val[12], test[12])}
    print(bar)
    return line, names


def progress(args, epoch, step, v):
    """The reference's line at step % 1000 == 0"""
    if args.predID == 0:
        print("epoch: %d step: %d [loss] %.6f [L1 loss] %.6f " % (epoch, step, v[0], v[1]))
    elif args.predID == 1:
        print("epoch: %d step: %d [loss] %.6f [b] %.6f %.6f %.6f [d] %.6f %.6f %.6f" % ((epoch, step) + tuple(v)))
    else:
        print("epoch: %d step: %d [loss] %.6f [q] %.6f [b] %.6f %.6f %.6f [d] %.6f %.6f %.6f" % ((epoch, step) + tuple(v)))


def main(argv=None):
    args = build_parser().parse_args(argv)
    pl = plan(args)
    import numpy as np
    import torch

    from . import dataset, engine as E, weights as W
    comp, out_dir, sets = pl["comp"], pl["out_dir"], pl["sets"]
    os.makedirs(out_dir, exist_ok=True)
    log = os.path.join(out_dir, "loss.txt")
    eng = E.Engine(args.device, weight_dir=args.modelDir, allow_synthetic_mtt=args.predID == 0)
    try:
        eng.set_precision(args.valPrecision)
        trainer = Trainer(eng, args, comp, pl["start"], args.device)
        partner = {"Q": read_weights(pl["start"]["Q"])} if args.predID == 1 else {}
        first = 0
        if args.resume:
            last = torch.load(os.path.join(out_dir, "last.pt"), map_location="cpu", weights_only=True)
            if last["seed"] != args.seed or sorted(last["nets"]) != sorted(trainer.nets):
                print("train_qbd: --resume: last.pt was written with --seed %d for the nets %s" % (last["seed"], sorted(last["nets"])), file=sys.stderr)
                return 2
            for kind, net in trainer.nets.items():
                net.load_state_dict(last["nets"][kind])
            trainer.optimizer.load_state_dict(last["optim"])
            first = last["epoch"] + 1
        else:
            with open(log, "a") as f:
                f.write(HEADERS[args.predID])
        train = dataset.DeviceDataset(eng, args.inputDir, comp, args.qp, "Train", args.predID, args.device, files=sets["Train"])
        print("Start Training ...")
        for epoch in range(first, args.epoch):
            group = trainer.optimizer.param_groups[0]
            group["lr"] = learning_rate(args.lr, epoch, args.dr, group["lr"])
            total = torch.zeros(trainer.nvalues, dtype=torch.float64, device=trainer.device)
            steps = 0
            for step, batch in enumerate(train.batches(args.batchSize, True, args.seed, epoch, args.maxSteps)):
                values = trainer.step(batch)
                total += values
                steps += 1
                if step % 1000 == 0:
                    progress(args, epoch, step, values.tolist())
            mean = (total / steps).tolist()
            val, test = validate(eng, args, comp, sets, trainer, partner)
            line, names = report(args, comp, epoch, mean, val, test)
            with open(log, "a") as f:
                f.write("".join(str(np.float64(s)) + "," for s in line) + "\n")
            for kind in trainer.nets:
                net = "%s_%s" % (comp, kind)
                W.save_pmpw(os.path.join(out_dir, W.ref_net_name(net) + "_%d.pmpw" % args.qp), net, args.qp, trainer.numpy_weights(kind),
                            source="train_qbd --predID %d, epoch %d" % (args.predID, epoch))
                if (epoch + 1) % args.saveEvery == 0:
                    torch.save({k: v.detach().cpu() for k, v in trainer.nets[kind].state_dict().items()}, os.path.join(out_dir, names[kind]))
            for kind, w in partner.items():
                net = "%s_%s" % (comp, kind)
                W.save_pmpw(os.path.join(out_dir, W.ref_net_name(net) + "_%d.pmpw" % args.qp), net, args.qp, w, source="the partner train_qbd validated with")
            torch.save({"nets": {k: {n: v.detach().cpu() for n, v in net.state_dict().items()} for k, net in trainer.nets.items()},
                        "optim": trainer.optimizer.state_dict(), "epoch": epoch, "seed": args.seed}, os.path.join(out_dir, "last.pt"))
    finally:
        eng.set_stream(0)
        eng.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
