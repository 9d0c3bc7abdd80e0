"""A labelled set validated in batches: what Metrics.validation_QBD / pre_validation of the reference compute, device-resident.

    read_set(...)                 the files of one set in the reference's layout, opened and checked (validate, train_qbd, dataset)
    run(engine, mode, ...)        the set through the nets (or given logits) in batches -> ValRun; Engine.validation_QBD and
                                  Engine.pre_validation are this call plus the rendering of their documented tuples (engine.py)
    ValRun                        the one result of a run: per-batch statistics, batch sizes, per-block partials, per-batch confusion
                                  counts; numbers() and confusion() are what the reference and the CLIs report; join / gathered put
                                  the runs of consecutive batch ranges (several ranks) together into the run of the whole set
    MODES, MODE_MAPS, NAMES ...   one table per fact about the three modes: "qbd" (both nets, validation_QBD), "q" (the QT net alone,
                                  pre_validation predID 0), "bd" (the MTT net teacher-forced, predID 1)
    validation_numbers, confusion_summary, _logit_label_arrays     statistics -> result lists, counts -> fractions, and the six
                                  optional arrays of val_stats / train_loss / val_confusion as the ABI takes them

Importing this module touches no GPU; torch is imported on use."""
import os
from types import SimpleNamespace

import numpy as np

from . import _lib

MODES = ("qbd", "q", "bd")
CONF_MAPS = ("qt", "bt0", "bt1", "bt2", "dire0", "dire1", "dire2")
HEADS = ("q", "b0", "b1", "b2", "d0", "d1", "d2")                           # the same seven maps in the reference's result names
VAL_ELEMS = np.array([64] + [256] * 12 + [64] + [256] * 6, np.float64)      # elements per block behind each of the twenty statistics
# Per mode: the maps it predicts as indices into CONF_MAPS.  Map i has its L1 sum in statistic i and its hit count in statistic 13 + i.
MODE_MAPS = {"qbd": (0, 1, 2, 3, 4, 5, 6), "q": (0,), "bd": (1, 2, 3, 4, 5, 6)}
HAS_LOSS = {"qbd": True, "q": False, "bd": True}                            # val_loss closes the list (pre_validation predID 0 has none)
COLS = {m: [i for i in maps] + [13 + i for i in maps] for m, maps in MODE_MAPS.items()}
NAMES = {m: [HEADS[i] + "_L1" for i in maps] + [HEADS[i] + "_accu" for i in maps] + ["val_loss"] * HAS_LOSS[m] for m, maps in MODE_MAPS.items()}


def mode_of_pred(pred_id):
    """The loader's PredID (train_qbd --predID) -> mode: 0 pre_train_Q, 1 pre_train_BD, 2 train_QBD"""
    return {0: "q", 1: "bd", 2: "qbd"}[pred_id]


class ValRun:
    """One validation run, or a batch range's share of one: mode, S float64[batches,20], ns (the batches' sizes), block_stats
    float64[N,20] or None (the set's rows, zeros outside the range), conf int64[batches,7,5,5] or None.  numbers(): the reference's
    result list of the mode (NAMES[mode]; ValueError for a run without batches); confusion(): the counts of all batches, int64[7,5,5]."""

    def __init__(self, mode, S, ns, block_stats=None, conf=None):
        self.mode, self.S, self.ns, self.block_stats, self.conf = mode, S, ns, block_stats, conf

    def numbers(self):
        return validation_numbers(self.S, self.ns, self.mode)

    def confusion(self):
        return self.conf.sum(axis=0)

    @staticmethod
    def join(runs):
        """Runs over consecutive batch ranges, in batch order -> the run of their union: the whole set's numbers and counts, bit for
        bit.  The per-block partials do not travel: ask the whole run for them."""
        runs = list(runs)
        conf = None if runs[0].conf is None else np.concatenate([r.conf for r in runs], 0)
        return ValRun(runs[0].mode, np.concatenate([r.S for r in runs], 0), [n for r in runs for n in r.ns], None, conf)

    def gathered(self, counts, device):
        """join over the ranks of a process group: this rank ran counts[rank] batches (parallel.shard_counts) -> every rank's run of
        the whole set, through grad_sync.gather_batch_stats."""
        from . import grad_sync
        S, ns, *conf = grad_sync.gather_batch_stats(self.S, self.ns, counts, device, conf=self.conf)
        return ValRun(self.mode, S, ns, None, conf[0] if conf else None)


def read_set(data_dir, data_type, comp, qp, with_mtt_labels, fail, with_blocks=True):
    """Opens (memory-mapped) and checks the files of one set of the reference's layout (validate.py's docstring) -> {"blocks": y or
    (y, u, v), "qt8", "msbt", "msdire" (None without with_mtt_labels), "n"}.  fail(message) is called on the first missing file, wrong
    dtype, wrong shape or mismatched count, and must not return.  Shared by validate, dataset.DeviceDataset and train_qbd.
    with_blocks=False: the labels alone, no block file is opened and "blocks" is None."""
    def read(name, dtype, tail):
        path = os.path.join(data_dir, name)
        if not os.path.isfile(path):
            fail("%s not found" % path)
        try:
            a = np.load(path, mmap_mode="r", allow_pickle=False)
        except (ValueError, OSError) as e:
            fail("%s: %s" % (path, e))
        if a.dtype != dtype or a.ndim != len(tail) + 1 or a.shape[1:] != tail:
            fail("%s: expected %s[n,%s], got %s%s" % (path, np.dtype(dtype).name, ",".join(map(str, tail)), a.dtype.name, list(a.shape)))
        return a
    stem = "%s_%s_QP%d_" % (data_type, comp, qp)
    out = {"qt8": read(stem + "QTdepth_Block8.npy", np.uint8, (8, 8)), "msbt": None, "msdire": None}
    n = out["qt8"].shape[0]
    if with_mtt_labels:
        out["msbt"] = read(stem + "MSBTdepth_Block16.npy", np.uint8, (3, 16, 16))
        out["msdire"] = read(stem + "MSdirection_Block16.npy", np.int8, (3, 16, 16))
    arrays = [("labels", out["msbt"]), ("labels", out["msdire"])]
    y = None
    if with_blocks:
        y = read(data_type + "_Y_Block68.npy", np.uint8, (68, 68))
        arrays.append(("blocks", y))
    if comp == "Chroma" and with_blocks:
        u = read(data_type + "_U_Block34.npy", np.uint8, (34, 34))
        v = read(data_type + "_V_Block34.npy", np.uint8, (34, 34))
        arrays += [("blocks", u), ("blocks", v)]
        out["blocks"] = (y, u, v)
    else:
        out["blocks"] = y
    for what, a in arrays:
        if a is not None and a.shape[0] != n:
            fail("%d %s for %d QT label blocks" % (a.shape[0], what, n))
    if n == 0:
        fail("the set is empty")
    out["n"] = n
    return out


# ---------------------------------------------------------------------------------------------- the run
def run(engine, mode, comp, qp, blocks, qt8, msbt, msdire, batch_size, logits=None, want_blocks=False, batch_range=None,
        want_confusion=False, group_blocks=16384):
    """The set (arguments as Engine.validation_QBD documents them) through `mode` in batches of batch_size -> ValRun; with batch_range =
    (lo, hi) only the set's batches lo .. hi-1 run and S, ns and conf are theirs.  Device-resident: per batch one inference call, one
    statistics call and, with want_confusion, one confusion call, all enqueued without waiting; the host synchronises once per GROUP of
    batches (at most group_blocks blocks, whose logits stay in device memory until then: a range-guard re-run at the synchronize finds
    every batch's buffers intact)."""
    import torch
    if comp not in ("Luma", "Chroma"):
        raise ValueError("comp must be 'Luma' or 'Chroma'")
    batch_size = int(batch_size)
    if batch_size < 1:
        raise ValueError("batch_size must be >= 1")
    dev = torch.device("cuda", int(engine.device))
    d = _upload(engine, mode, comp, qp, blocks, qt8, msbt, msdire, logits, dev)
    starts, ns, groups = _plan(d.n, batch_size, batch_range, group_blocks)
    S = torch.zeros((len(starts), _lib.PMP_VAL_NSTATS), dtype=torch.float64, device=dev)
    blk = torch.zeros((d.n, _lib.PMP_VAL_NSTATS), dtype=torch.float64, device=dev) if want_blocks else None
    conf = torch.zeros((len(starts), _lib.PMP_CONF_NCOUNTS), dtype=torch.int64, device=dev) if want_confusion else None
    torch.cuda.synchronize(dev)                       # the uploads above ran on torch's stream; the context has its own
    for grp in groups:
        base = starts[grp[0]]
        l = _group_logits(d, base, sum(ns[i] for i in grp), dev)
        for i in grp:
            _enqueue(engine, mode, comp, qp, d, l, starts[i], ns[i], starts[i] - base, _at(S, i, _lib.PMP_VAL_NSTATS, 8),
                     _at(blk, starts[i], _lib.PMP_VAL_NSTATS, 8), _at(conf, i, _lib.PMP_CONF_NCOUNTS, 8))
        engine.synchronize()                          # final: range flags looked at, re-runs and their statistics replayed
    return ValRun(mode, S.cpu().numpy(), ns, None if blk is None else blk.cpu().numpy(), None if conf is None else
                  conf.cpu().numpy().reshape(-1, _lib.PMP_CONF_MAPS, _lib.PMP_CONF_CLASSES, _lib.PMP_CONF_CLASSES))


_at = lambda t, row, width, elem: None if t is None else t.data_ptr() + row * width * elem    # device pointer to a row of width elements of elem bytes


def _to_device(a, dev):
    import torch
    return torch.from_numpy(np.array(a, copy=not a.flags.writeable or not a.flags.c_contiguous)).to(dev)   # memory-mapped files are read-only


def _upload(engine, mode, comp, qp, blocks, qt8, msbt, msdire, logits, dev):
    """Step 1: check the set against the mode, load the nets it runs, and upload it -> the set on the device: n, use = which of
    (qt, bt, dire) the mode has, q8 / mb / md the labels, y / u / v the blocks and qin the teacher-forced mode's QT input (None with
    logits given), logits = the host arrays (qt, bt, dire) as [n, 64 | 768] rows, None for what the mode leaves out (None: the nets run)."""
    use_q, use_m = mode in ("qbd", "q"), mode in ("qbd", "bd")
    qt8 = _fit(qt8, np.uint8, "qt8")
    n = qt8.size // 64
    if qt8.size != n * 64:
        raise ValueError("qt8 must be u8[N,8,8]")
    if use_m:
        if msbt is None or msdire is None:
            raise ValueError("msbt and msdire labels are needed")
        msbt = _fit(msbt, np.uint8, "msbt"); msdire = _fit(msdire, np.int8, "msdire")
        if msbt.size != n * 768 or msdire.size != n * 768:
            raise ValueError("msbt and msdire must be [N,3,16,16] for the N blocks of qt8")
    d = SimpleNamespace(n=n, use=(use_q, use_m, use_m), y=None, u=None, v=None, qin=None, logits=None)
    if logits is None:
        by, bu, bv = (blocks if isinstance(blocks, (tuple, list)) else (blocks, None, None))
        by, bu, bv = (None if a is None else np.ascontiguousarray(a, dtype=np.uint8) for a in (by, bu, bv))
        if engine._check_blocks(comp, by, bu, bv) != n:
            raise ValueError("%d blocks for %d label blocks" % (by.shape[0], n))
        engine.load(comp, qp, kinds=("Q",) if mode == "q" else ("Q", "MSBD"))
        d.y = _to_device(by, dev)
        if comp == "Chroma":
            d.u, d.v = _to_device(bu, dev), _to_device(bv, dev)
    else:
        want = (64,) * use_q + (768, 768) * use_m
        logits = [np.ascontiguousarray(a, np.float32) for a in logits]
        if len(logits) != len(want) or any(a.size != n * w for a, w in zip(logits, want)):
            raise ValueError("logits: expected %d arrays of N x %s floats" % (len(want), "/".join(map(str, want))))
        it = iter(a.reshape(n, w) for a, w in zip(logits, want))
        d.logits = [next(it) if use else None for use in d.use]
    d.q8 = _to_device(qt8, dev)
    d.mb = _to_device(msbt, dev) if use_m else None
    d.md = _to_device(msdire, dev) if use_m else None
    if mode == "bd" and logits is None:               # the loader's label map: float(u8(qt8 - 1))
        d.qin = _to_device((qt8 - np.uint8(1)).astype(np.float32), dev)
    return d


def _plan(n, batch_size, batch_range, group_blocks):
    """Step 2: n blocks in batches of batch_size, in order -> (starts, the first block of every batch that runs; ns, their sizes, the
    last one of the set ragged; groups, lists of indices into these, of at most group_blocks blocks and at least one batch each)."""
    starts = list(range(0, n, batch_size))
    if batch_range is not None:
        lo, hi = int(batch_range[0]), int(batch_range[1])
        if not 0 <= lo <= hi <= len(starts):
            raise ValueError("batch_range must lie in 0 .. %d" % len(starts))
        starts = starts[lo:hi]
    ns = [min(batch_size, n - o) for o in starts]
    per_group = max(1, int(group_blocks) // batch_size)
    return starts, ns, [list(range(g0, min(g0 + per_group, len(starts)))) for g0 in range(0, len(starts), per_group)]


def _group_logits(d, base, m, dev):
    """The logits (qt, bt, dire) of one group, blocks base .. base+m-1, as device tensors, None for what the mode leaves out: buffers
    for the nets to fill, or those rows of the logits given."""
    import torch
    if d.logits is None:
        return [torch.empty((m, w), dtype=torch.float32, device=dev) if use else None for use, w in zip(d.use, (64, 768, 768))]
    l = [None if a is None else _to_device(a[base:base + m], dev) for a in d.logits]
    torch.cuda.synchronize(dev)                       # uploads on torch's stream again, ahead of the context's
    return l


def _enqueue(engine, mode, comp, qp, d, l, o, m, r, d_stats, d_block_stats, d_conf):
    """Step 3: one batch, blocks o .. o+m-1 of the set d, whose logits are rows r .. r+m-1 of the group's l: the mode's inference call
    where the nets run, the statistics call, and the confusion call where d_conf is given.  Nothing waits."""
    l_q, l_b, l_d = _at(l[0], r, 64, 4), _at(l[1], r, 768, 4), _at(l[2], r, 768, 4)
    if d.logits is None:
        yuv = (_at(d.y, o, 68 * 68, 1), _at(d.u, o, 34 * 34, 1), _at(d.v, o, 34 * 34, 1))
        if mode == "bd":
            engine.infer_msbd_device(comp, qp, *yuv, _at(d.qin, o, 64, 4), m, l_b, l_d)
        elif mode == "q":
            engine.infer_q_device(comp, qp, *yuv, m, l_q)
        else:
            engine.infer_device(comp, qp, *yuv, m, l_q, l_b, l_d)
    six = (l_q, l_b, l_d, _at(d.q8, o, 64, 1) if d.use[0] else None, _at(d.mb, o, 768, 1), _at(d.md, o, 768, 1))
    engine.val_stats_device(qp, *six, m, d_stats, d_block_stats)
    if d_conf is not None:
        engine.val_confusion_device(*six, m, d_conf)


# ---------------------------------------------------------------------------------------------- arrays in, numbers out
def _fit(a, dtype, name):
    """a as a contiguous array of `dtype` if every value fits it exactly (the reference's label dtypes); ValueError otherwise."""
    a = np.asarray(a)
    if a.dtype == dtype:
        return np.ascontiguousarray(a)
    info = np.iinfo(dtype)
    if a.dtype.kind not in "biuf":
        raise ValueError("%s: numeric array expected, got %s" % (name, a.dtype))
    if a.size and (a.dtype.kind == "f" and not np.all(np.isfinite(a) & (a == np.round(a)))
                   or a.min() < info.min or a.max() > info.max):
        raise ValueError("%s: values outside %s (the reference's dtype); refusing to wrap them" % (name, np.dtype(dtype).name))
    return np.ascontiguousarray(a.astype(dtype))


def _logit_label_arrays(qt, bt, dire, qt8, msbt, msdire, census=False):
    """The six optional arrays of val_stats / train_loss / val_confusion as the ABI takes them: contiguous float32 logits, labels in the
    reference's dtypes (u8, u8, i8) if every value fits exactly.  The QT pair (qt, qt8), the MTT four (bt, dire, msbt, msdire) or both;
    census (val_confusion): a group's labels may also come without its logits.  -> ((qt, bt, dire, qt8, msbt, msdire), block count);
    ValueError on a mix the ABI refuses or on sizes that disagree."""
    f = lambda a: None if a is None else np.ascontiguousarray(a, np.float32)
    fit = lambda a, dtype, name: None if a is None else _fit(a, dtype, name)
    qt, bt, dire, qt8, msbt, msdire = arrays = (f(qt), f(bt), f(dire), fit(qt8, np.uint8, "qt8"), fit(msbt, np.uint8, "msbt"), fit(msdire, np.int8, "msdire"))
    torn = (bt is None) != (dire is None) or (msbt is None) != (msdire is None) or qt is not None and qt8 is None or bt is not None and msbt is None
    if torn or not census and (qt is None and qt8 is not None or bt is None and msbt is not None) or qt8 is None and msbt is None:
        raise ValueError("logits and labels: pass (qt, qt8), (bt, dire, msbt, msdire) or both%s" % ("; a group's labels may come alone" if census else ""))
    n = (qt8.size // 64) if qt8 is not None else (msbt.size // 768)
    if any(a is not None and a.size != n * w for a, w in zip(arrays, (64, 768, 768, 64, 768, 768))):
        raise ValueError("logits and labels: expected qt, qt8 [N,8,8] and bt, dire, msbt, msdire [N,3,16,16] for one N")
    return arrays, n


def confusion_summary(C):
    """What confusion counts int64[7,5,5] (pmp_val_confusion: C[m][label class][predicted class]) say, per map: {map name: {"matrix":
    the 5x5 counts as lists, "total", "label_freq": row sums / total (depth maps: the classes 0..3 and other; direction maps: -1, 0, 1,
    other, and a fifth class that stays empty), and as fractions of the total
      depth maps (qt, bt0..2)      "hit" p == l, "under" p < l (splits the encoder can no longer try), "over" p > l (splits it did not
                                   want) - label and prediction both one of 0..3;
      direction maps (dire0..2)    "hit", "missed" (l != 0, p == 0), "false" (l == 0, p != 0), "flipped" (l == -p != 0) - both one of -1, 0, 1;
      both                         "other_label" (the label is no valid class), "other_pred" (the label is, the prediction is not)}}.
    A map without cells (a group that was not given) has total 0 and zeros for every fraction."""
    C = np.asarray(C, np.int64).reshape(_lib.PMP_CONF_MAPS, _lib.PMP_CONF_CLASSES, _lib.PMP_CONF_CLASSES)
    out = {}
    for m, name in enumerate(CONF_MAPS):
        M = C[m]
        nv = 4 if m < 4 else 3                            # valid classes; the rest is "other"
        V = M[:nv, :nv]
        total = int(M.sum())
        parts = {"hit": int(np.trace(V))}
        if m < 4:
            parts["under"] = int(np.tril(V, -1).sum())
            parts["over"] = int(np.triu(V, 1).sum())
        else:
            parts["missed"] = int(V[0, 1] + V[2, 1])
            parts["false"] = int(V[1, 0] + V[1, 2])
            parts["flipped"] = int(V[0, 2] + V[2, 0])
        parts["other_label"] = int(M[nv:, :].sum())
        parts["other_pred"] = int(M[:nv, nv:].sum())
        assert sum(parts.values()) == total
        d = {"matrix": M.tolist(), "total": total, "label_freq": [(int(v) / total if total else 0.0) for v in M.sum(axis=1)]}
        d.update({k: (v / total if total else 0.0) for k, v in parts.items()})
        out[name] = d
    return out


def validation_numbers(S, ns, mode="qbd"):
    """The reference's result lists from per-batch statistics S float64[batches,20] (include/pmp.h: pmp_val_stats) of batches of ns
    blocks: "qbd" -> validation_QBD's 15, "q" -> pre_validation predID 0's [L1, accuracy], "bd" -> predID 1's 13 (NAMES).  A per-batch
    L1 is S / elements, an accuracy hits / elements, the loss loss_func_QBD_val (without the QT term for "bd"); np.mean over the batches."""
    S = np.asarray(S, np.float64).reshape(-1, _lib.PMP_VAL_NSTATS)
    nb = np.asarray(ns, np.float64).reshape(-1, 1)
    if len(S) == 0:
        raise ValueError("validation of an empty set")
    with np.errstate(invalid="ignore"):
        R = S / (VAL_ELEMS[None, :] * nb)
        loss = (0.8 * S[:, 1] + 1.0 * S[:, 2] + 1.2 * S[:, 3] + S[:, 7] + S[:, 8] + S[:, 9] + 0.5 * (S[:, 10] + S[:, 11] + S[:, 12])) / (256.0 * nb[:, 0])
        if mode == "qbd":
            loss = S[:, 0] / (64.0 * nb[:, 0]) + loss
        out = [float(np.mean(R[:, j])) for j in COLS[mode]]
        if HAS_LOSS[mode]:
            out.append(float(np.mean(loss)))
    return out
