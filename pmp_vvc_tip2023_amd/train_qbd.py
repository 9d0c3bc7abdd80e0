"""Train_QBD.py's three training modes on this library, resident on the GPU.

    python -m pmp_vvc_tip2023_amd.train_qbd --predID 0|1|2 [--isLuma] --inputDir D --outDir O [--jobID 0000] [--lr 1e-3] [--dr 20]
           [--qp 22] [--epoch 100] [--batchSize 200] [--lambq .. --lambresb2 ..]
           [--modelDir M] [--seed 0] [--saveEvery 10] [--resume] [--maxSteps K] [--device 0] [--valPrecision f16x3|bf16x6|fp32]
           [--gpus N] [--microBatch 256] [--clipNorm X] [--skipNonFinite] [--maxSkipped 10] [--confusion]

--predID 0 is pre_train_Q (the QT net on the plain L1 loss, Train_QBD.py:117-191), 1 is pre_train_BD (the MTT net teacher-forced with
the QT labels on loss_func_MSBD, :193-303), 2 is train_QBD (both nets jointly on loss_func_QBD, starting from the pair <comp>_Q_<qp> and
<comp>_BD_<qp> (.pmpw or .pkl) in --modelDir, :305-429).  The reference's flags keep their names and defaults.  --inputDir holds the
three sets Train, Validate and TestSub in the reference's file names (validate.py's docstring); results go to <outDir>/<jobID>/.

A step: the learning rate by Metrics.adjust_learning_rate's rule, a batch gathered on the device (dataset.DeviceDataset), the nets'
forward (q_net.QNet, msbd_net.MSBDNet), the loss (train_loss), backward(), optim.Adam.step() - one launch.  A batch of more than
--microBatch blocks (1..256, the most the training calls take) runs as micro-batches of at most that many whose losses are weighted
n_i / n and whose gradients add up in .grad, so --batchSize 400 works.  The numbers the reference reads with .item() at every step
come from the loss call's thirteen sums and are added up on the device; the host reads them once per epoch and at step % 1000 == 0
for the progress line.

An epoch ends as the reference's: Engine.pre_validation / Engine.validation_QBD of the current parameters (loaded into the engine
with Engine.load_pretrain_model, on the --valPrecision datapath) on the Validate and TestSub sets, the reference's printed lines, and
one line of loss.txt under the reference's header: an epoch value is the mean of the step values.  Every --saveEvery epochs the
checkpoints are written under the reference's names (<comp>_Q_<qp>_epoch_%d_....pkl, <comp>_BD_...: plain state_dicts,
weights.load_pkl reads them), and at every epoch <comp>_Q_<qp>.pmpw / <comp>_BD_<qp>.pmpw of the nets as they are now - the directory
then serves as --modelDir of inference_qbd and validate - and last.pt (nets, optimiser, epoch, seed), from which --resume continues.
--predID 1 also writes the QT net it validated with as <comp>_Q_<qp>.pmpw, so that the pair is whole.  --predID 0 validates through
Engine.infer_q: the QT net alone is loaded and run, no *_BD_* file is looked for and no stand-in takes its place.

--confusion: every epoch's validation also counts, per map of the mode (0: qt; 1: bt0..2, dire0..2; 2: all seven), the joint histogram
of (label class, predicted class) (include/pmp.h: pmp_val_confusion; validation.confusion_summary reads it) and appends one line per set
and map, "epoch,set,map,c00,c01,..,c44" (set Validate or TestSub, cLP = label class L, predicted class P), to confusion.txt.  Without
the flag nothing is counted or written.  Under --gpus N the per-batch counts travel with the per-batch statistics and the file is the
one-rank run's, byte for byte.

--gpus N (or torchrun's environment, as inference_qbd) trains data-parallel, the reference's nn.DataParallel: N rank processes
(parallel.spawn_ranks), each on the GPU of its LOCAL_RANK (--device is refused; ranks share a GPU only under PMP_DIST_BACKEND=gloo, for
tests), every rank holding the whole Train set and the same permutation, taking rows [r*m, min((r+1)*m, n)) of each batch, m =
ceil(batchSize / N) <= --microBatch, and the ranks' gradients added in rank order by grad_sync.GradSync.  The run writes, byte for byte,
the files of the one-rank run with --microBatch m.  Validate and TestSub are dealt out batch-wise (parallel.shard_bounds) and their
per-batch statistics gathered in batch order.  Rank 0 alone prints and writes; --resume loads on every rank.  Before the first step
and after every epoch the ranks compare a fingerprint of their parameters: a mismatch ends the job with status 4.  The speed-up has
not been measured: no multi-GPU node was available, and ranks that share one GPU (gloo) show the bits, not the time.

THE DIVERGENCE GUARD, off by default (without its flags every file and bit is what it was): --clipNorm X clips the step's gradients
by their global norm as torch.nn.utils.clip_grad_norm_(parameters, X) would; --skipNonFinite makes a step whose gradients hold a NaN
or an inf write nothing to any parameter or moment (optim.Adam's max_grad_norm and skip_nonfinite: one pmp_grad_guard_device call per
step, the decision taken and obeyed on the device).  A skipped step still counts as a step (optim.py).  With either flag a skipped step's
values are masked out of the epoch's totals on the device and the epoch means are over the steps taken.  The host reads the guard's
counters where it already reads: at step % 1000 == 0 and at the epoch's end.  If more than --maxSkipped steps in a row were skipped
(meaningful only with --skipNonFinite), or no step of the epoch was taken, the job ends with exit status 5 and a message naming the epoch
and the counters - BEFORE validation and before any .pmpw, .pkl or last.pt is written, so the files of the last good epoch stay.  Every
epoch appends "epoch,steps,skipped,clipped,max_run,max_norm" - the counters since the job's first step, max_norm the largest gradient
norm seen - to guard.txt; last.pt carries them under "guard" and --resume restores them.  Under --gpus N every rank sees the same
gradient bits behind GradSync.sync, takes the same decisions and returns the same status; rank 0 writes guard.txt, whose bytes are the
one-rank run's too.

What differs from the reference: the order of the batches is defined by --seed (dataset.permutation of (seed, epoch): a resumed run
gives the bits of an uninterrupted one); processes instead of nn.DataParallel's threads (state_dict names without "module.");
micro-batches.
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
MICRO_MAX = 256                         # the largest n the training calls take
EXIT_DESYNC = 4                         # the ranks' parameters differ
EXIT_DIVERGED = 5                       # the divergence guard ended the job


class _Given(argparse.Action):
    """Stores the value and, as <dest>Given, that the flag stood on the command line"""

    def __call__(self, parser, namespace, values, option_string=None):
        setattr(namespace, self.dest, values)
        setattr(namespace, self.dest + "Given", True)


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
    p.add_argument("--device", default=0, type=int, action=_Given, help="GPU of a one-rank run; with several ranks each takes that of its LOCAL_RANK")
    p.set_defaults(deviceGiven=False)
    p.add_argument("--gpus", default=1, type=int,
                   help="train data-parallel on this many GPUs of the node: started without a launcher the command spawns its own rank "
                        "processes; under torchrun it is one rank")
    p.add_argument("--microBatch", default=MICRO_MAX, type=int, help="blocks per forward and backward pass at most, 1..256")
    p.add_argument("--clipNorm", default=0.0, type=float, help="clip the gradients' global norm to this; 0: off")
    p.add_argument("--skipNonFinite", action="store_true", help="a step whose gradients hold a NaN or an inf changes nothing")
    p.add_argument("--maxSkipped", default=10, type=int, help="with --skipNonFinite: more skipped steps in a row end the job with status 5")
    p.add_argument("--confusion", action="store_true", help="append the validation's confusion counts per set and map to confusion.txt")
    p.add_argument("--valPrecision", default="f16x3", help="datapath of the validation passes: f16x3, bf16x6 or fp32")
    return p


def learning_rate(lr, epoch, decay_rate, current):
    """Metrics.adjust_learning_rate (Metrics.py:53-57): lr * 0.5 ** (epoch // decay_rate) if that is above 1e-6, else the current one."""
    adj = lr * (0.5 ** (epoch // decay_rate))
    return adj if adj > 1e-6 else current


def plan(args):
    """Checks every flag, opens the three sets (validation.read_set) and finds the model files -> {"comp", "sets": {name: read_set's
    dict}, "start": {net: (kind, path)} of --predID 2's pair, "out_dir"}.  SystemExit(2) on the first problem, nothing has touched the GPU."""
    from . import _lib, weights as W
    from .grad_sync import rank_share
    from .validation import read_set

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
    if not 1 <= args.microBatch <= MICRO_MAX:
        fail("--microBatch must be in 1 .. %d" % MICRO_MAX)
    if not (math.isfinite(args.clipNorm) and args.clipNorm >= 0):
        fail("--clipNorm must be finite and >= 0 (0: no clipping)")
    if args.maxSkipped < 0:
        fail("--maxSkipped must be >= 0")
    if not 1 <= args.gpus <= _lib.PMP_GRAD_SUM_MAX:
        fail("--gpus must be in 1 .. %d" % _lib.PMP_GRAD_SUM_MAX)
    world = job_world(args)[1]
    if world > 1:
        if world > _lib.PMP_GRAD_SUM_MAX:
            fail("at most %d ranks" % _lib.PMP_GRAD_SUM_MAX)
        if args.deviceGiven:
            fail("--device selects the GPU of a one-rank run; with %d ranks every rank takes the GPU of its LOCAL_RANK" % world)
        if rank_share(args.batchSize, world) > args.microBatch:
            fail("--batchSize %d on %d ranks is %d blocks a rank, more than --microBatch %d" %
                 (args.batchSize, world, rank_share(args.batchSize, world), args.microBatch))
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


def job_world(args):
    """(rank, world, local rank): torchrun's environment where there is one, else rank 0 of --gpus (the parent that spawns them)"""
    from . import parallel
    return parallel.env_world() if "WORLD_SIZE" in os.environ else (0, args.gpus, 0)


def rank_device(args, world, local):
    """The GPU of this rank, by inference_qbd.open_job's rule: --device on one rank; with several the LOCAL_RANK's, and a GPU
    shared by several ranks only under PMP_DIST_BACKEND=gloo"""
    if world == 1:
        return args.device
    import torch
    ndev = torch.cuda.device_count()
    if local < ndev:
        return local
    if os.environ.get("PMP_DIST_BACKEND", "nccl") == "nccl":
        raise SystemExit("rank with LOCAL_RANK %d of %d has no GPU of its own (%d visible): RCCL needs one GPU per rank "
                         "(PMP_DIST_BACKEND=gloo lets several ranks share a GPU, for tests only)" % (local, world, ndev))
    return local % max(ndev, 1)


def guard_kwargs(args):
    """optim.Adam's guard arguments for the flags: none at their defaults, which leaves the optimiser on its unguarded path"""
    kw = {}
    if getattr(args, "clipNorm", 0.0):
        kw["max_grad_norm"] = args.clipNorm
    if getattr(args, "skipNonFinite", False):
        kw["skip_nonfinite"] = True
    return kw


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
        self.optimizer = optim.Adam(engine, [p for net in self.nets.values() for p in net.parameters()], lr=args.lr, **guard_kwargs(args))
        self.nvalues = {0: 2, 1: 7, 2: 8}[args.predID]
        self.sync, self.world = None, 1
        self.guarded = bool(guard_kwargs(args))
        self.taken = None                                 # guarded: the steps taken since begin_epoch(), an int64 device scalar

    def begin_epoch(self):
        import torch
        if self.guarded:
            self.taken = torch.zeros((), dtype=torch.int64, device=self.device)

    def data_parallel(self):
        """Call once the process group stands: from here on step() adds the ranks' gradients and numbers (grad_sync.GradSync)"""
        from . import grad_sync
        self.sync = grad_sync.GradSync(self.engine, [p for net in self.nets.values() for p in net.parameters()], self.device)
        self.world = self.sync.world

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

    def accumulate(self, batch, n=None):
        """zero_grad, then forward and backward of the batch in micro-batches of at most --microBatch blocks -> step_values.  The .grads
        hold the gradient of the whole batch's loss.  n: the batch is this rank's rows (None: no row) of a batch of n, whose loss
        the rows are weighted for; the values and the .grads are then this rank's terms of the batch's."""
        import torch
        self.optimizer.zero_grad(set_to_none=True)
        rows = 0 if batch is None else batch[0].shape[0]
        n = rows if n is None else n
        micro = self.args.microBatch
        values = torch.zeros(self.nvalues, dtype=torch.float64, device=self.device)
        for s in range(0, rows, micro):
            part = tuple(t[s:s + micro] for t in batch)
            w = part[0].shape[0] / n
            loss, l1 = self.forward_loss(part)
            (loss * w if w != 1.0 else loss).backward()
            values[0] += loss.detach().double() * w
            values[1:] += l1 / n
        return values

    def step(self, batch, n=None):
        """One step on a whole batch or, data-parallel, on this rank's rows of a batch of n (dataset.rank_batches) -> step_values of
        the whole batch, the same on every rank.  Guarded: zeros for a step the guard skipped, and self.taken counts the others"""
        values = self.accumulate(batch, n)
        if self.sync is not None:
            from .grad_sync import active_ranks
            n = batch[0].shape[0] if n is None else n
            values = self.sync.sync(active_ranks(n, self.args.batchSize, self.world), values)
        self.optimizer.step()
        if self.guarded:
            import torch
            if self.taken is None:
                self.begin_epoch()
            taken = self.optimizer.step_taken
            values = torch.where(taken, values, torch.zeros_like(values))
            self.taken += taken
        return values

    def fingerprint(self):
        """weights.fingerprint of every parameter and buffer of the nets"""
        from . import weights as W
        return W.fingerprint({kind + "." + k: v for kind in self.nets for k, v in self.numpy_weights(kind).items()})

    def numpy_weights(self, kind):
        return {k: v.detach().cpu().numpy() for k, v in self.nets[kind].state_dict().items()}


def validate(engine, args, comp, sets, trainer, partner):
    """The epoch's validation: the current parameters into the engine, then validation.run on Validate and TestSub -> their two
    ValRuns (with --confusion they carry the counts).  Data-parallel (trainer.sync): the batches of each set are dealt out by
    parallel.shard_bounds, a rank runs its own, and the runs, gathered in rank order, which is batch order, are the same on every rank."""
    from . import parallel, validation
    for kind in trainer.nets:
        engine.load_pretrain_model("%s_%s" % (comp, kind), args.qp, trainer.numpy_weights(kind))
    for kind, w in partner.items():
        if not engine.has_weights("%s_%s" % (comp, kind), args.qp):
            engine.load_pretrain_model("%s_%s" % (comp, kind), args.qp, w)
    out = []
    for name in SETS[1:]:
        d, sync = sets[name], trainer.sync
        nb = -(-d["n"] // args.batchSize)
        run = validation.run(engine, validation.mode_of_pred(args.predID), comp, args.qp, d["blocks"], d["qt8"], d["msbt"], d["msdire"],
                             args.batchSize, batch_range=parallel.shard_bounds(nb, sync.rank, sync.world) if sync is not None else None,
                             want_confusion=bool(getattr(args, "confusion", False)))
        if sync is not None:
            run = run.gathered(parallel.shard_counts(nb, sync.world), trainer.device)
        out.append(run)
    return out


def confusion_lines(epoch, runs):
    """The epoch's lines of confusion.txt: per set (Validate, TestSub) and map of the mode "epoch,set,map,c00..c44" """
    from .validation import CONF_MAPS, MODE_MAPS
    lines = []
    for name, run in zip(SETS[1:], runs):
        conf = run.confusion()
        lines += ["%d,%s,%s,%s\n" % (epoch, name, CONF_MAPS[m], ",".join(str(int(v)) for v in conf[m].ravel())) for m in MODE_MAPS[run.mode]]
    return "".join(lines)


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


def launch_ranks(n, argv):
    """--gpus N without a launcher: N fresh rank processes of this command (the parent makes no GPU call), all of them watched: the
    first rank that fails ends the job with its exit code (parallel.spawn_ranks)."""
    from . import parallel
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    rc, _ = parallel.spawn_ranks([sys.executable, "-m", "pmp_vvc_tip2023_amd.train_qbd"] + list(argv), n,
                                 env_extra={"PYTHONPATH": root + os.pathsep + os.environ.get("PYTHONPATH", "")})
    return rc


def open_group(device, world):
    """The rendezvous, its preflight collective and the steady-state timeout, as inference_qbd's ranks -> whether a process group
    stands (several ranks, or one forced with PMP_DIST_FORCE=1)"""
    import torch
    import torch.distributed as dist
    from . import parallel
    torch.cuda.set_device(device)
    parallel.init_process_group(device)
    if world > 1:
        parallel.preflight(device)
        parallel.relax_timeout()
    return dist.is_initialized()


def in_sync(trainer, when):
    """The desync check: every rank's fingerprint of its parameters against rank 0's -> True, or False behind a message naming the ranks"""
    from . import grad_sync
    bad = grad_sync.ranks_out_of_sync(trainer.fingerprint(), trainer.device)
    if bad:
        print("train_qbd: %s the parameters of rank %s differ from rank 0's: the ranks have run apart (seen by rank %d)" %
              (when, ", ".join(map(str, bad)), trainer.sync.rank), file=sys.stderr, flush=True)
    return not bad


def diverged(args, epoch, counters, taken):
    """The guard's verdict where the host reads -> None, or the message the job ends with (status EXIT_DIVERGED).  taken: the
    steps of the epoch that were taken, None within an epoch"""
    if counters["max_run"] <= args.maxSkipped and taken != 0:
        return None
    why = "no step of the epoch was taken" if taken == 0 else "%d steps in a row were skipped (--maxSkipped %d)" % (counters["max_run"], args.maxSkipped)
    return "train_qbd: diverged in epoch %d: %s; counters: %s.  Nothing of this epoch was written" % (
        epoch, why, ", ".join("%s %s" % (k, counters[k]) for k in ("steps", "skipped", "clipped", "run", "max_run", "max_norm")))


def main(argv=None):
    argv = sys.argv[1:] if argv is None else list(argv)
    args = build_parser().parse_args(argv)
    pl = plan(args)
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        return launch_ranks(args.gpus, argv)
    import numpy as np
    import torch

    from . import dataset, engine as E, weights as W
    comp, out_dir, sets = pl["comp"], pl["out_dir"], pl["sets"]
    rank, world, local = job_world(args)
    dev_id = rank_device(args, world, local)
    say = print if rank == 0 else (lambda *a, **k: None)
    if rank == 0:
        os.makedirs(out_dir, exist_ok=True)
    log = os.path.join(out_dir, "loss.txt")
    eng = E.Engine(dev_id, weight_dir=args.modelDir)
    try:
        eng.set_precision(args.valPrecision)
        trainer = Trainer(eng, args, comp, pl["start"], dev_id)
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
            if trainer.guarded and "guard" in last:
                trainer.optimizer.load_guard_state(last["guard"])
            first = last["epoch"] + 1
        elif rank == 0:
            with open(log, "a") as f:
                f.write(HEADERS[args.predID])
        if (world > 1 or os.environ.get("PMP_DIST_FORCE") == "1") and open_group(trainer.device, world):
            trainer.data_parallel()
            if not in_sync(trainer, "before the first step"):
                return EXIT_DESYNC
        train = dataset.DeviceDataset(eng, args.inputDir, comp, args.qp, "Train", args.predID, dev_id, files=sets["Train"])
        say("Start Training ...")
        for epoch in range(first, args.epoch):
            group = trainer.optimizer.param_groups[0]
            group["lr"] = learning_rate(args.lr, epoch, args.dr, group["lr"])
            total = torch.zeros(trainer.nvalues, dtype=torch.float64, device=trainer.device)
            steps = 0
            trainer.begin_epoch()
            if trainer.sync is None:
                batches = ((None, b) for b in train.batches(args.batchSize, True, args.seed, epoch, args.maxSteps))
            else:
                batches = train.rank_batches(args.batchSize, rank, world, True, args.seed, epoch, args.maxSteps)
            for step, (n, batch) in enumerate(batches):
                values = trainer.step(batch, n)
                total += values
                steps += 1
                if step % 1000 == 0 and rank == 0:
                    progress(args, epoch, step, values.tolist())
                if step % 1000 == 0 and trainer.guarded:            # every rank reads, and every rank reads the same
                    bad = diverged(args, epoch, trainer.optimizer.guard_state(), None)
                    if bad:
                        print(bad, file=sys.stderr, flush=True)
                        return EXIT_DIVERGED
            counters = None
            if trainer.guarded:
                counters, steps = trainer.optimizer.guard_state(), int(trainer.taken)
                bad = diverged(args, epoch, counters, steps)
                if bad:
                    print(bad, file=sys.stderr, flush=True)
                    return EXIT_DIVERGED
            mean = (total / steps).tolist()
            runs = validate(eng, args, comp, sets, trainer, partner)
            if trainer.sync is not None and not in_sync(trainer, "after epoch %d" % epoch):
                return EXIT_DESYNC
            if rank != 0:
                continue
            line, names = report(args, comp, epoch, mean, *[r.numbers() for r in runs])
            with open(log, "a") as f:
                f.write("".join(str(np.float64(s)) + "," for s in line) + "\n")
            if runs[0].conf is not None:
                with open(os.path.join(out_dir, "confusion.txt"), "a") as f:
                    f.write(confusion_lines(epoch, runs))
            if counters is not None:
                with open(os.path.join(out_dir, "guard.txt"), "a") as f:
                    f.write("%d,%d,%d,%d,%d,%s\n" % (epoch, counters["steps"], counters["skipped"], counters["clipped"], counters["max_run"],
                                                    repr(float(counters["max_norm"]))))
            for kind in trainer.nets:
                net = "%s_%s" % (comp, kind)
                W.save_pmpw(os.path.join(out_dir, W.ref_net_name(net) + "_%d.pmpw" % args.qp), net, args.qp, trainer.numpy_weights(kind),
                            source="train_qbd --predID %d, epoch %d" % (args.predID, epoch))
                if (epoch + 1) % args.saveEvery == 0:
                    torch.save({k: v.detach().cpu() for k, v in trainer.nets[kind].state_dict().items()}, os.path.join(out_dir, names[kind]))
            for kind, w in partner.items():
                net = "%s_%s" % (comp, kind)
                W.save_pmpw(os.path.join(out_dir, W.ref_net_name(net) + "_%d.pmpw" % args.qp), net, args.qp, w, source="the partner train_qbd validated with")
            last = {"nets": {k: {n: v.detach().cpu() for n, v in net.state_dict().items()} for k, net in trainer.nets.items()},
                    "optim": trainer.optimizer.state_dict(), "epoch": epoch, "seed": args.seed}
            if counters is not None:
                last["guard"] = counters
            torch.save(last, os.path.join(out_dir, "last.pt"))
        if trainer.sync is not None:
            import torch.distributed as dist
            dist.barrier()
            dist.destroy_process_group()
    finally:
        eng.set_stream(0)
        eng.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
