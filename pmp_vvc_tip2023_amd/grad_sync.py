"""Data-parallel training whose result is defined bit for bit: what nn.DataParallel is to Train_QBD.py (:130, :207, :325-326), one
process per GPU (torch.distributed, parallel.py), with the ranks' gradients added IN RANK ORDER by a kernel of this library
(pmp_grad_sum_device, include/pmp.h TRAINING STEP) where an all-reduce would add them in an order that belongs to the communication
library.  A step on W ranks is then, bit for bit, the step of one rank whose micro-batches are the ranks' slices:

    rows of a batch of n    rank r takes [r*m, min((r+1)*m, n)), m = ceil(batchSize / W)                       rank_rows
    loss                    a rank weighs its loss by n_r / n, as a micro-batch does                           train_qbd.Trainer
    gradients               every rank packs its .grads into one bucket (pmp_grad_pack_device), the buckets of all ranks are
                            gathered (all_gather_into_tensor on RCCL; through CPU tensors on gloo), every rank adds the buckets
                            of the ACTIVE ranks ((b0 + b1) + b2 ..., as torch's AccumulateGrad adds micro-batches), and every
                            parameter's .grad becomes a view of that sum: optim.Adam.step() runs unchanged        GradSync.sync
    reported numbers        the float64 vector of Trainer.accumulate, gathered and added in rank order in the same way

The divergence guard (optim.Adam's max_grad_norm / skip_nonfinite, train_qbd --clipNorm / --skipNonFinite) needs nothing here:
behind GradSync.sync every .grad is a view into the summed bucket, so the table pmp_grad_guard_device walks has the same counts in the
same order on every rank and on one rank, and its census is defined by counts and order alone, not by where a tensor lies.  The guard
therefore sees the same bits on every rank - a NaN that one rank's slice produced is in every rank's sum - and every rank takes the
same decision, the one the one-rank run with --microBatch m takes (tests/test_gpu_train_qbd_guard.py, two ranks against one).

A rank whose slice of a ragged batch is empty is not active: it packs zeros, takes part in the gather, and is left out of the sum,
because x + 0.0 is not x for x = -0.0.  Rank 0 is active in every step.  Which parameters have a gradient at all is rank 0's pattern,
exchanged once: the others get .grad = None, as on one rank, and Adam skips them.

What this cannot show on one GPU is the speed-up: several ranks share a device only through the gloo backend (PMP_DIST_BACKEND=gloo),
which is for tests.  No multi-GPU node was available; no scaling number is claimed anywhere.
torch is imported on use."""
from . import _lib
from .torch_call import P, run


def rank_share(batch_size, world):
    """m: the rows of a full batch one rank takes"""
    return -(-int(batch_size) // int(world))


def rank_rows(n, batch_size, rank, world):
    """The rows [lo, hi) of a batch of n <= batch_size rows that `rank` of `world` takes; hi == lo: none (a ragged last batch)."""
    n, batch_size, rank, world = int(n), int(batch_size), int(rank), int(world)
    if world < 1 or not 0 <= rank < world or batch_size < 1 or not 0 <= n <= batch_size:
        raise ValueError("rank_rows: bad arguments")
    m = rank_share(batch_size, world)
    return min(rank * m, n), min((rank + 1) * m, n)


def active_ranks(n, batch_size, world):
    """The ranks that take at least one row of a batch of n, ascending: 0 .. ceil(n / m) - 1"""
    return [r for r in range(world) if rank_rows(n, batch_size, r, world)[1] > rank_rows(n, batch_size, r, world)[0]]


def all_gather_rows(local):
    """Every rank's tensor `local` (one shape and dtype on all ranks) -> [world, *local.shape] on local's device, row r from rank r.
    RCCL moves device tensors; gloo moves CPU tensors, as parallel.all_reduce_sum does."""
    import torch
    import torch.distributed as dist
    world = dist.get_world_size()
    if dist.get_backend() == "nccl":
        out = torch.empty((world,) + tuple(local.shape), dtype=local.dtype, device=local.device)
        dist.all_gather_into_tensor(out, local.contiguous())
        return out
    cpu = local.detach().cpu().contiguous()
    slots = [torch.empty_like(cpu) for _ in range(world)]
    dist.all_gather(slots, cpu)
    return torch.stack(slots).to(local.device)


def gather_batch_stats(S, ns, counts, device, conf=None):
    """Validation on several ranks: this rank's per-batch statistics S float64[k, 20] and batch sizes ns[k], k = counts[rank] (the
    batches dealt out by parallel.shard_bounds) -> (S float64[sum(counts), 20], ns) of all ranks in rank order, which is batch order.
    validation.ValRun.gathered is the caller.  conf: this rank's per-batch confusion counts int64[k, 7, 5, 5] (pmp_val_confusion) travel with the statistics, in the same rows -
    a batch's count is far below 2^53, so float64 carries it exactly - and come back as a third element int64[sum(counts), 7, 5, 5]."""
    import numpy as np
    import torch
    cap = max(max(counts), 1)
    nc = _lib.PMP_CONF_NCOUNTS if conf is not None else 0
    mine = np.zeros((cap, _lib.PMP_VAL_NSTATS + 1 + nc), np.float64)
    mine[:len(ns), :_lib.PMP_VAL_NSTATS] = np.asarray(S, np.float64).reshape(-1, _lib.PMP_VAL_NSTATS)
    mine[:len(ns), _lib.PMP_VAL_NSTATS] = ns
    if nc:
        mine[:len(ns), _lib.PMP_VAL_NSTATS + 1:] = np.asarray(conf, np.int64).reshape(-1, nc)
    every = all_gather_rows(torch.from_numpy(mine).to(device)).cpu().numpy()
    rows = np.concatenate([every[r, :c] for r, c in enumerate(counts)], 0)
    out = (rows[:, :_lib.PMP_VAL_NSTATS].copy(), [int(v) for v in rows[:, _lib.PMP_VAL_NSTATS]])
    if nc:
        out += (rows[:, _lib.PMP_VAL_NSTATS + 1:].astype(np.int64).reshape(-1, _lib.PMP_CONF_MAPS, _lib.PMP_CONF_CLASSES, _lib.PMP_CONF_CLASSES),)
    return out


def ranks_out_of_sync(fingerprint, device):
    """The ranks whose 64-bit parameter fingerprint (weights.fingerprint) differs from rank 0's, ascending; [] when all agree."""
    import torch
    fp = int(fingerprint) & ((1 << 64) - 1)
    halves = torch.tensor([fp >> 32, fp & 0xFFFFFFFF], dtype=torch.int64, device=device)
    every = all_gather_rows(halves).cpu().tolist()
    return [r for r, v in enumerate(every) if v != every[0]]


class GradSync:
    """One bucket for this rank's gradients and one receive area for all ranks', for the parameters `params` (a list in one order on
    every rank) on `device`.  Needs an initialised process group (a forced one-rank group runs the same calls)."""

    def __init__(self, engine, params, device):
        import torch
        import torch.distributed as dist
        from .engine import grad_bucket_floats
        self.engine, self.params, self.device = engine, list(params), device
        self.rank, self.world = dist.get_rank(), dist.get_world_size()
        if self.world > _lib.PMP_GRAD_SUM_MAX:
            raise ValueError("GradSync: at most %d ranks" % _lib.PMP_GRAD_SUM_MAX)
        for p in self.params:
            if p.dtype != torch.float32 or p.device != device or not p.is_contiguous():
                raise ValueError("GradSync: parameters must be contiguous float32 tensors on %s" % device)
        self.counts = [p.numel() for p in self.params]
        self.total, self.offsets = grad_bucket_floats(self.counts)
        self.bucket = torch.empty(self.total, dtype=torch.float32, device=device)
        self.recv = torch.empty((self.world, self.total), dtype=torch.float32, device=device)
        self.nccl = dist.get_backend() == "nccl"
        self.has_grad = None                      # rank 0's pattern, exchanged in the first sync

    def _pattern(self, mine):
        import torch
        import torch.distributed as dist
        t = torch.tensor(mine, dtype=torch.uint8, device=self.device if self.nccl else "cpu")
        dist.broadcast(t, src=0)
        return [bool(v) for v in t.cpu().tolist()]

    def sync(self, active, values=None):
        """active: the ranks whose slice of this step's batch is not empty, ascending, the same list on every rank.  -> the sum of the
        active ranks' `values` (a 1-D device tensor of one length on all ranks) in rank order, from zero, or None.  Afterwards every
        parameter's .grad is a view of the sum of the active ranks' gradients (None where no rank has one), until the next sync."""
        import torch
        import torch.distributed as dist
        active = list(active)
        if not active or active != sorted(set(active)) or active[0] < 0 or active[-1] >= self.world:
            raise ValueError("GradSync.sync: active must name ranks of the group, ascending")
        grads = [None if p.grad is None else p.grad.detach().to(torch.float32).contiguous() for p in self.params]
        mine = [g is not None for g in grads]
        if self.has_grad is None:
            self.has_grad = self._pattern(mine)
        if mine != (self.has_grad if self.rank in active else [False] * len(mine)):
            raise RuntimeError("GradSync: rank %d's parameters with a gradient differ from rank 0's first step" % self.rank)
        run(self.engine, self.device, lambda: self.engine.grad_pack_device([P(g) for g in grads], self.counts, P(self.bucket)))
        if self.nccl:
            dist.all_gather_into_tensor(self.recv, self.bucket)
        else:
            self.recv.copy_(all_gather_rows(self.bucket))
        total = self.recv[active[0]]                  # the sum in place: d_dst = d_src[0]
        run(self.engine, self.device, lambda: self.engine.grad_sum_device([P(self.recv[r]) for r in active], self.total, P(total)))
        for p, off, count, has in zip(self.params, self.offsets, self.counts, self.has_grad):
            p.grad = total[off:off + count].view_as(p) if has else None
        if values is None:
            return None
        every = all_gather_rows(values)
        out = torch.zeros_like(values)
        for r in active:
            out += every[r]
        return out
