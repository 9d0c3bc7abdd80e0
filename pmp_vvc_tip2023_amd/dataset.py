"""Metrics.Load_Pre_VP_Dataset (Metrics.py:64-146) resident on the GPU: the set is uploaded ONCE as the uint8 / int8 the .npy files
hold (6.5 KB a luma block against the 18.5 KB of the reference's host-side float32 tensors) and every batch is assembled there by one
pmp_batch_gather_device call (include/pmp.h, TRAINING STEP) - no DataLoader, no workers, no copy per step.

    train = DeviceDataset(engine, args.inputDir, "Luma", args.qp, "Train", pred_id=2, device=0)
    for x, qt_f, msbt, msdire, qt8 in train.batches(args.batchSize, shuffle=True, seed=args.seed, epoch=epoch): ...

Files, dtypes, shapes and counts are checked by validation.read_set, the reader validate.plan uses.  pred_id as the loader's PredID: 0
yields (x, qt_f, qt8) - the QT labels alone are read - 1 and 2 yield (x, qt_f, msbt, msdire, qt8): the loader's tuple with the label
tensors in the dtypes of the label FILES, as train_loss takes them, and the raw qtDepth rows beside the loader's float(qt8 - 1).  x is
f32[n,1,68,68] (Luma) or f32[n,3,34,34] (Chroma: the 2x2 maximum of Y, U, V).  Batches are cut from one permutation of the set in
order, the last one ragged, as DataLoader(shuffle=True, drop_last=False) cuts them.  The permutation is torch.randperm of a CPU
generator seeded by (seed, epoch) and nothing else, uploaded once per epoch: an epoch's batches do not depend on what ran before it.
The gather's status word (an index outside the set) is read once, behind the epoch's last batch, and raises.  The tensors of a batch
are fresh: the caller may keep them.  torch is imported on use."""
import numpy as np

from . import _lib
from .torch_call import P, run
from .validation import read_set


def epoch_seed(seed, epoch):
    """The generator seed of (seed, epoch): distinct for distinct pairs of 0 <= epoch < 2^20."""
    return (int(seed) << 20) + int(epoch)


def permutation(n, shuffle, seed, epoch):
    """The order of an epoch: torch.randperm(n) of a CPU generator seeded by epoch_seed, or 0..n-1 -> int64 CPU tensor"""
    import torch
    if not shuffle:
        return torch.arange(n, dtype=torch.int64)
    return torch.randperm(n, generator=torch.Generator().manual_seed(epoch_seed(seed, epoch)), dtype=torch.int64)


class DeviceDataset:
    def __init__(self, engine, data_dir, comp, qp, data_type, pred_id, device=0, files=None):
        """files: what read_set returned for these arguments, if the caller has already opened them (train_qbd.plan)."""
        import torch
        if pred_id not in (0, 1, 2):
            raise ValueError("pred_id must be 0, 1 or 2")

        def fail(msg):
            raise ValueError(msg)
        d = files if files is not None else read_set(data_dir, data_type, comp, int(qp), pred_id != 0, fail)
        self.engine, self.comp, self.pred_id, self.n = engine, comp, pred_id, d["n"]
        self.device = torch.device("cuda", int(device))
        # memory-mapped files are read-only: torch wants a writable array
        up = lambda a: None if a is None else torch.from_numpy(np.array(a, copy=not a.flags.writeable or not a.flags.c_contiguous)).to(self.device)
        y, u, v = d["blocks"] if comp == "Chroma" else (d["blocks"], None, None)
        self.t = {"y": up(y), "u": up(u), "v": up(v), "qt8": up(d["qt8"]), "msbt": up(d["msbt"]), "msdire": up(d["msdire"])}
        self.src = _lib.BatchSrc(*[P(self.t[k]) for k in ("y", "u", "v", "qt8", "msbt", "msdire")], self.n)
        self.status = torch.zeros(1, dtype=torch.int32, device=self.device)

    def gather(self, d_index, n):
        """The rows d_index (an int64 device tensor, or a view of one) names -> the batch's tuple, from one library call."""
        import torch
        new = lambda shape, dt: torch.empty(shape, dtype=dt, device=self.device)
        x = new((n, 3, 34, 34) if self.comp == "Chroma" else (n, 1, 68, 68), torch.float32)
        qt_f = new((n, 1, 8, 8), torch.float32)
        mtt = self.pred_id != 0
        qt8 = new((n, 8, 8), torch.uint8)
        msbt = new((n, 3, 16, 16), torch.uint8) if mtt else None
        msdire = new((n, 3, 16, 16), torch.int8) if mtt else None
        run(self.engine, self.device, lambda: self.engine.batch_gather_device(
            self.src, P(d_index), n, P(self.status), d_x=P(x), d_qt_f=P(qt_f), d_qt8=P(qt8), d_msbt=P(msbt), d_msdire=P(msdire)))
        return (x, qt_f, msbt, msdire, qt8) if mtt else (x, qt_f, qt8)

    def _indices(self, batch_size, shuffle, seed, epoch, max_batches):
        """The index tensors of the epoch's batches, views of one permutation on the device"""
        batch_size = int(batch_size)
        if not 1 <= batch_size <= _lib.PMP_BATCH_MAX:
            raise ValueError("batch_size must be in 1 .. %d" % _lib.PMP_BATCH_MAX)
        order = permutation(self.n, shuffle, seed, epoch).to(self.device)
        count = (self.n + batch_size - 1) // batch_size
        for b in range(count if max_batches is None else min(count, int(max_batches))):
            yield order[b * batch_size:(b + 1) * batch_size]

    def batches(self, batch_size, shuffle=True, seed=0, epoch=0, max_batches=None):
        """Yields the epoch's batches (at most max_batches of them); raises behind the last one if any index lay outside the set."""
        for idx in self._indices(batch_size, shuffle, seed, epoch, max_batches):
            yield self.gather(idx, idx.numel())
        self.check()

    def rank_batches(self, batch_size, rank, world, shuffle=True, seed=0, epoch=0, max_batches=None):
        """The same epoch on `world` ranks (grad_sync.py): every rank derives the same permutation and gathers only its own rows of
        each batch, grad_sync.rank_rows.  Yields (n, rows): the size of the WHOLE batch and this rank's tuple, None where the rank
        takes no row of a ragged batch."""
        from .grad_sync import rank_rows
        for idx in self._indices(batch_size, shuffle, seed, epoch, max_batches):
            lo, hi = rank_rows(idx.numel(), batch_size, rank, world)
            yield idx.numel(), (self.gather(idx[lo:hi], hi - lo) if hi > lo else None)
        self.check()

    def check(self):
        """Reads the status word (this waits for the gathers enqueued so far) and raises if one of them met an index outside the set."""
        if int(self.status.item()):
            self.status.zero_()
            raise RuntimeError("DeviceDataset: a batch index lay outside the set of %d blocks; its rows were zeros" % self.n)
