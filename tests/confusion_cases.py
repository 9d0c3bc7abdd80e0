"""Confusion counts (include/pmp.h: pmp_val_confusion): a numpy restatement of the rule and the cases the CPU and GPU tests share.

The rule: counts[m][l][p] = number of cells of map m (0 qt, 1..3 bt_k, 4..6 dire_k) whose label has class l and whose prediction
r = round-half-to-even(logit) has class p.  Class of a value v, label or r alike: on a depth map v if v is one of 0, 1, 2, 3, else 4;
on a direction map v + 1 if v is one of -1, 0, 1, else 3.  Labels are converted as the loader converts them: ql = float(u8(qt8 - 1))."""
import numpy as np

MAPS, CLASSES, NCOUNTS = 7, 5, 175
NAMES = ("qt", "bt0", "bt1", "bt2", "dire0", "dire1", "dire2")
ORDER = ("qt", "bt", "dire", "qt8", "msbt", "msdire")


def depth_class(v):
    """v float array holding integers, NaN or +-inf -> int class 0..4"""
    v = np.asarray(v, np.float64)
    out = np.full(v.shape, 4, np.int64)
    for k in range(4):
        out[v == k] = k                      # -0.0 == 0; NaN equals nothing
    return out


def dire_class(v):
    v = np.asarray(v, np.float64)
    out = np.full(v.shape, 3, np.int64)
    for k in (-1, 0, 1):
        out[v == k] = k + 1
    return out


def predicted(x):
    """torch.round / rintf: half to even (np.rint is), NaN and inf pass through"""
    with np.errstate(invalid="ignore"):
        return np.rint(np.asarray(x, np.float32)).astype(np.float64)


def _hist(l, p):
    h = np.zeros((CLASSES, CLASSES), np.int64)
    np.add.at(h, (l.ravel(), p.ravel()), 1)
    return h


def block_counts(qt=None, bt=None, dire=None, qt8=None, msbt=None, msdire=None):
    """-> int64[n, 7, 5, 5], each block on its own.  A group's labels without its logits: the census (every prediction "other")."""
    n = len(qt8) if qt8 is not None else len(msbt)
    out = np.zeros((n, MAPS, CLASSES, CLASSES), np.int64)
    for b in range(n):
        if qt8 is not None:
            ql = (np.asarray(qt8[b], np.uint8) - np.uint8(1)).astype(np.float64)
            l = depth_class(ql)
            p = depth_class(predicted(np.reshape(qt[b], ql.shape))) if qt is not None else np.full(l.shape, 4)
            out[b, 0] = _hist(l, p)
        if msbt is not None:
            for k in range(3):
                lb = depth_class(np.asarray(msbt[b, k], np.float64))
                ld = dire_class(np.asarray(msdire[b, k], np.float64))
                pb = depth_class(predicted(bt[b, k])) if bt is not None else np.full(lb.shape, 4)
                pd = dire_class(predicted(dire[b, k])) if dire is not None else np.full(ld.shape, 3)
                out[b, 1 + k] = _hist(lb, pb)
                out[b, 4 + k] = _hist(ld, pd)
    return out


def counts(**kw):
    return block_counts(**kw).sum(axis=0)


def diagonal(C):
    """Hits per map over the VALID classes: what S[13..19] of pmp_val_stats count when every label is a valid class"""
    C = np.asarray(C).reshape(MAPS, CLASSES, CLASSES)
    return np.array([np.trace(C[m][:4, :4]) if m < 4 else np.trace(C[m][:3, :3]) for m in range(MAPS)], np.int64)


def in_range(n, seed):
    """Random logits around in-range labels (qt8 raw 1..4 -> labels 0..3, msbt 0..3, msdire -1..1): every label is a valid class, so
    the diagonal is the reference's hit count."""
    rng = np.random.default_rng(seed)
    qt8 = rng.integers(1, 5, (n, 8, 8)).astype(np.uint8)
    msbt = rng.integers(0, 4, (n, 3, 16, 16)).astype(np.uint8)
    msdire = rng.integers(-1, 2, (n, 3, 16, 16)).astype(np.int8)
    noise = lambda shape: (rng.standard_normal(shape) * 0.7).astype(np.float32)
    qt = (qt8.astype(np.float32) - 1 + noise(qt8.shape)).astype(np.float32)
    bt = (msbt.astype(np.float32) + noise(msbt.shape)).astype(np.float32)
    dire = (msdire.astype(np.float32) + noise(msdire.shape)).astype(np.float32)
    # exact halves, which round to even, among them
    for a in (qt, bt, dire):
        flat = a.reshape(-1)
        at = rng.choice(flat.size, max(1, flat.size // 16), replace=False)
        flat[at] = np.floor(flat[at]) + 0.5
    return dict(qt=qt, bt=bt, dire=dire, qt8=qt8, msbt=msbt, msdire=msdire)


# (logit, expected class on a depth map, expected class on a direction map); 4 / 3 = "other"
NAN, INF = float("nan"), float("inf")
SPECIAL_LOGITS = [(0.5, 0, 1), (1.5, 2, 3), (2.5, 2, 3), (3.5, 4, 3), (-0.4, 0, 1), (-0.5, 0, 1), (-0.51, 4, 0), (NAN, 4, 3), (INF, 4, 3),
                  (-INF, 4, 3), (1e30, 4, 3), (-0.0, 0, 1), (0.49999997, 0, 1), (-1.5, 4, 3), (-1.4999, 4, 0), (2.9, 3, 3)]
SPECIAL_QT8 = [(0, 4), (5, 4), (1, 0), (4, 3), (255, 4)]            # raw 0 -> label 255; raw 5 -> label 4
SPECIAL_MSBT = [(4, 4), (200, 4), (0, 0), (3, 3)]
SPECIAL_MSDIRE = [(2, 3), (-128, 3), (-1, 0), (0, 1), (1, 2), (127, 3), (-2, 3)]


def special(n=2, seed=5):
    """n blocks of in-range data with the special logits and labels written over the first cells of every map of every block; each
    special logit meets each special label once in block 0 (the qt map has room for 64 pairs, the others for 256)."""
    c = in_range(n, seed)
    lq = [x for x, _, _ in SPECIAL_LOGITS]
    pairs_q = [(x, r) for r, _ in SPECIAL_QT8 for x in lq][:64]
    for i, (x, r) in enumerate(pairs_q):
        c["qt"].reshape(n, 64)[0, i] = x
        c["qt8"].reshape(n, 64)[0, i] = r
    pairs_b = [(x, r) for r, _ in SPECIAL_MSBT for x in lq]
    pairs_d = [(x, r) for r, _ in SPECIAL_MSDIRE for x in lq]
    for k in range(3):
        for i, (x, r) in enumerate(pairs_b):
            c["bt"].reshape(n, 3, 256)[0, k, i] = x
            c["msbt"].reshape(n, 3, 256)[0, k, i] = r
        for i, (x, r) in enumerate(pairs_d):
            c["dire"].reshape(n, 3, 256)[0, k, i] = x
            c["msdire"].reshape(n, 3, 256)[0, k, i] = r
    return c


FORMS = {"both": ORDER, "q": ("qt", "qt8"), "m": ("bt", "dire", "msbt", "msdire"), "census": ("qt8", "msbt", "msdire"),
         "q+census_m": ("qt", "qt8", "msbt", "msdire"), "census_q+m": ("qt8", "bt", "dire", "msbt", "msdire"), "census_q": ("qt8",),
         "census_m": ("msbt", "msdire")}


def form(c, name, s=slice(None)):
    return {k: c[k][s] for k in FORMS[name]}


def file_lines(epoch, confs, maps, sets=("Validate", "TestSub")):
    """train_qbd's confusion.txt lines of one epoch"""
    return "".join("%d,%s,%s,%s\n" % (epoch, name, NAMES[m], ",".join(str(int(v)) for v in C[m].ravel())) for name, C in zip(sets, confs)
                   for m in maps)
