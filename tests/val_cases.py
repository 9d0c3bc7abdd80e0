"""Seeded inputs of the validation-statistics tests and a plain numpy restatement of the twenty numbers (include/pmp.h: pmp_val_stats).

Test infrastructure, not product.  The restatement is written from the formulas of the header: float32 terms in the reference's order,
float64 sums.  tools/gen_golden_val.py feeds the same cases to the REFERENCE (Metrics.validation_QBD, pre_validation, loss_func_*_val)
and stores its numbers in tests/golden/g12_val.npz; the inputs are rebuilt here from their seeds.
"""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g12_val.npz")
NSTATS = 20
ELEMS = np.array([64] + [256] * 12 + [64] + [256] * 6, np.float64)
SUMS, COUNTS = list(range(13)), list(range(13, 20))
WEIGHT_MAT = 0.5 * np.array([[1.0, 0.73, 0.15], [2.43, 0.35, 0.10], [0.96, 0.23, 0.07], [0.59, 0.16, 0.05]])   # Metrics.py:148-151

# name -> (qp, blocks, batch size, seed, non-finite logits).  Batches are cut in order; every case has a ragged tail.
CASES = {
    "qp22": (22, 450, 200, 2201, False),
    "qp27": (27, 450, 200, 2701, False),
    "qp32": (32, 330, 128, 3201, False),
    "qp37": (37, 450, 200, 3701, False),
    "qp41_small": (41, 37, 16, 4101, False),
    "nonfinite": (27, 150, 64, 9901, True),
}


def labels(n, seed):
    """qt8 u8[n,8,8] RAW qtDepth 0..4 (0 included: the loader's u8 subtraction turns it into 255), msbt u8[n,3,16,16] non-decreasing
    over the layers, msdire i8[n,3,16,16] in {-1, 0, 1}."""
    rng = np.random.default_rng(seed)
    qt8 = rng.integers(0, 5, (n, 8, 8)).astype(np.uint8)
    qt8[::7, 0, 0] = 0
    step = rng.integers(0, 2, (n, 3, 16, 16))
    msbt = np.cumsum(step, axis=1).astype(np.uint8)
    msdire = rng.integers(-1, 2, (n, 3, 16, 16)).astype(np.int8)
    return qt8, msbt, msdire


def _specials():
    """Exact k + 0.5 of both parities and both signs, +-0.5, and the float32 neighbours one ulp either side of a half."""
    halves = np.array([0.5, 1.5, 2.5, 3.5, 4.5, -0.5, -1.5, -2.5, 254.5, 255.5], np.float32)
    up = np.nextafter(halves, np.float32(np.inf), dtype=np.float32)
    dn = np.nextafter(halves, np.float32(-np.inf), dtype=np.float32)
    return np.concatenate([halves, up, dn, np.array([0.0, -0.0, 1.0, 255.0], np.float32)])


def make(name):
    """-> dict(qp, n, batch, qt f32[n,8,8], bt f32[n,3,16,16], dire f32[n,3,16,16], qt8, msbt, msdire)."""
    qp, n, batch, seed, nonfinite = CASES[name]
    qt8, msbt, msdire = labels(n, seed)
    rng = np.random.default_rng(seed + 1)
    ql = (qt8 - np.uint8(1)).astype(np.float32)
    qt = (ql + rng.normal(0, 0.45, ql.shape)).astype(np.float32)
    bt = (msbt + rng.normal(0, 0.45, msbt.shape)).astype(np.float32)
    dire = (msdire + rng.normal(0, 0.45, msdire.shape)).astype(np.float32)
    sp = _specials()
    for a in (qt, bt, dire):                       # specials scattered over every map, every batch
        flat = a.reshape(-1)
        idx = rng.choice(flat.size, size=min(flat.size // 8, 40 * len(sp)), replace=False)
        flat[idx] = sp[np.arange(len(idx)) % len(sp)]
    if nonfinite:                                   # in the first and the last (ragged) batch only: the middle batch stays finite
        for b in (3, n - 2):
            qt[b, 1, 2] = np.nan
            bt[b, 0, 3, 4] = np.inf
            bt[b + 1, 2, 0, 0] = -np.inf
            dire[b, 1, 5, 6] = -np.inf
            dire[b, 2, 7, 8] = np.nan
    return {"qp": qp, "n": n, "batch": batch, "qt": qt, "bt": bt, "dire": dire, "qt8": qt8, "msbt": msbt, "msdire": msdire}


def batches(c):
    return [(o, min(c["batch"], c["n"] - o)) for o in range(0, c["n"], c["batch"])]


def loader_labels(qt8, msbt, msdire):
    """The loader's conversions (Metrics.py:127-135): ql = float(qt8 - 1) with numpy's u8 subtraction, bl = float(msbt), dl = float(msdire)."""
    return (qt8 - np.uint8(1)).astype(np.float32), msbt.astype(np.float32), msdire.astype(np.float32)


def weights(qp, dl):
    """w_k f32[n,16,16] for k = 0..2: dl_k*dl_k + float32(weight_mat[row][k]); w_0 = 1.0 when qp == 22."""
    row = WEIGHT_MAT[int((qp - 22) / 5)]
    w = [dl[:, k] * dl[:, k] + np.float32(row[k]) for k in range(3)]
    if qp == 22:
        w[0] = np.ones_like(w[0])
    return w


def block_stats(qp, qt=None, bt=None, dire=None, qt8=None, msbt=None, msdire=None):
    """The twenty numbers per block, float64[n,20]: float32 terms, each block's terms added in float64."""
    n = len(qt) if qt is not None else len(bt)
    S = np.zeros((n, NSTATS), np.float64)
    f64sum = lambda t: t.reshape(n, -1).astype(np.float64).sum(axis=1)
    cnt = lambda x, lab: (np.round(x) == lab).reshape(n, -1).sum(axis=1).astype(np.float64)   # np.round: half to even; NaN never equal
    with np.errstate(invalid="ignore", over="ignore"):
        if qt is not None:
            ql = (qt8 - np.uint8(1)).astype(np.float32)
            q = qt.reshape(n, 8, 8).astype(np.float32)
            S[:, 0] = f64sum(np.abs(q - ql))
            S[:, 13] = cnt(q, ql)
        if bt is not None:
            bl, dl = msbt.astype(np.float32), msdire.astype(np.float32)
            w = weights(qp, dl)
            for k in range(3):
                S[:, 1 + k] = f64sum(np.abs(bt[:, k] - bl[:, k]))
                S[:, 4 + k] = f64sum(np.abs(dire[:, k] - dl[:, k]))
                S[:, 7 + k] = f64sum(np.abs(w[k] * dire[:, k] - w[k] * dl[:, k]))
                if k == 0:
                    S[:, 10] = f64sum(np.abs(w[0] * bt[:, 0] - w[0] * bl[:, 0]))
                else:
                    S[:, 10 + k] = f64sum(np.abs(w[k] * (bt[:, k] - bt[:, k - 1]) - w[k] * (bl[:, k] - bl[:, k - 1])))
                S[:, 14 + k] = cnt(bt[:, k], bl[:, k])
                S[:, 17 + k] = cnt(dire[:, k], dl[:, k])
    return S


def stats(qp, **kw):
    """The twenty numbers of one batch, float64[20]."""
    with np.errstate(invalid="ignore"):
        return block_stats(qp, **kw).sum(axis=0)


def case_stats(c, mode="qbd"):
    """Per-batch statistics float64[batches,20] of a case, batches cut in order; mode "q" / "bd": the QT-only / MTT-only form."""
    rows = []
    for o, m in batches(c):
        s = slice(o, o + m)
        kw = {}
        if mode in ("qbd", "q"):
            kw.update(qt=c["qt"][s], qt8=c["qt8"][s])
        if mode in ("qbd", "bd"):
            kw.update(bt=c["bt"][s], dire=c["dire"][s], msbt=c["msbt"][s], msdire=c["msdire"][s])
        rows.append(stats(c["qp"], **kw))
    return np.stack(rows), [m for _, m in batches(c)]


def numbers(S, ns, mode="qbd"):
    """The reference's result lists from per-batch statistics: validation_QBD's 15 ("qbd"), pre_validation's 2 ("q") or 13 ("bd")."""
    S = np.asarray(S, np.float64)
    nb = np.asarray(ns, np.float64)
    with np.errstate(invalid="ignore"):
        R = S / (ELEMS[None, :] * nb[:, None])
        loss = (0.8 * S[:, 1] + 1.0 * S[:, 2] + 1.2 * S[:, 3] + S[:, 7] + S[:, 8] + S[:, 9] + 0.5 * (S[:, 10] + S[:, 11] + S[:, 12])) / (256.0 * nb)
        if mode == "qbd":
            loss = S[:, 0] / (64.0 * nb) + loss
        cols = {"qbd": [0, 1, 2, 3, 4, 5, 6, 13, 14, 15, 16, 17, 18, 19], "q": [0, 13], "bd": [1, 2, 3, 4, 5, 6, 14, 15, 16, 17, 18, 19]}[mode]
        out = [np.mean(R[:, j]) for j in cols]
        if mode != "q":
            out.append(np.mean(loss))
    return np.array(out, np.float64), loss


# which entries of the result lists are ratios of integers (accuracies): exact against the reference
EXACT = {"qbd": list(range(7, 14)), "q": [1], "bd": list(range(6, 12))}


def rel_dist(a, b):
    """Largest relative distance over the entries where both are finite (NaN / inf entries must agree in kind: asserted)."""
    a, b = np.asarray(a, np.float64).ravel(), np.asarray(b, np.float64).ravel()
    fin = np.isfinite(a) & np.isfinite(b)
    assert np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(a[~fin & ~np.isnan(a)], b[~fin & ~np.isnan(b)]), (a, b)
    if not fin.any():
        return 0.0
    den = np.maximum(np.abs(b[fin]), np.finfo(np.float64).tiny)
    return float(np.max(np.abs(a[fin] - b[fin]) / den))
