"""Seeded inputs of the training-loss tests and a plain numpy restatement of include/pmp.h: pmp_train_loss.

Test infrastructure, not product.  The restatement is written from the header: float32 terms in the reference's order, float64 sums in
the kernel's fixed order (so a comparison with the GPU is bit for bit), the float64 loss in its written order, and gradients computed in
float64 and rounded once to float32.  tools/gen_golden_train_loss.py feeds the same cases to the REFERENCE (Train_QBD.loss_func_QBD,
loss_func_MSBD, L1_Loss, and torch's backward pass) and stores its numbers in tests/golden/g14_train_loss.npz; the inputs are rebuilt
here from their seeds.
"""
import os

import numpy as np

import val_cases as V

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g14_train_loss.npz")
NTERMS = 13
KEYS = ("lambq", "lambb0", "lambb1", "lambb2", "lambd0", "lambd1", "lambd2", "lambresb0", "lambresb1", "lambresb2")
DEFAULT = dict(zip(KEYS, (1.0, 0.8, 1.0, 1.2, 1.0, 1.0, 1.0, 0.5, 0.5, 0.5)))                     # Train_QBD.py:448-457
ZEROS_NEG = dict(zip(KEYS, (0.7, 0.0, 1.0, -0.25, 1.0, 0.0, 2.0, 0.5, 0.0, 1.5)))                 # zeros, a negative value, lambq != 1
CUSTOM = dict(zip(KEYS, (2.5, 0.3, 0.9, 1.1, 0.6, 1.7, 0.2, 0.45, 0.8, 0.05)))
LUMA_MAT = V.WEIGHT_MAT                                                                           # Train_QBD.py:35-38
CHROMA_MAT = 0.5 * np.array([[17.83, 0.49, 0.11], [1.20, 0.25, 0.07], [0.58, 0.17, 0.05], [0.38, 0.12, 0.04]])   # Train_QBD.py:39-42
MODES = ("qbd", "bd", "q")                      # loss_func_QBD, loss_func_MSBD, pre_train_Q's L1

# name -> (comp, qp, blocks, seed, loss weights, non-finite logits, passes of the host form).  40 blocks in all.
CASES = {
    "luma22_n1": ("Luma", 22, 1, 1401, DEFAULT, False, None),
    "chroma22_n1": ("Chroma", 22, 1, 1402, CUSTOM, False, None),
    "chroma27_n3": ("Chroma", 27, 3, 1403, ZEROS_NEG, False, None),
    "luma27_n2_nonfinite": ("Luma", 27, 2, 1407, ZEROS_NEG, True, None),
    "chroma32_n1_nonfinite": ("Chroma", 32, 1, 1408, DEFAULT, True, None),
    "luma37_n3": ("Luma", 37, 3, 1404, DEFAULT, False, None),
    "luma30_n17": ("Luma", 30, 17, 1405, CUSTOM, False, None),         # qp 30: row 1 through int(8 / 5); 17 = 16 row groups + 1
    "chroma41_5_5_2": ("Chroma", 41, 12, 1406, ZEROS_NEG, False, (5, 5, 2)),
}


def make(name):
    """-> dict(comp, qp, n, lam, passes, qt f32[n,8,8], bt, dire f32[n,3,16,16], qt8 u8, msbt u8, msdire i8)."""
    comp, qp, n, seed, lam, nonfinite, passes = CASES[name]
    qt8, msbt, msdire = V.labels(n, seed)          # raw qt8 0 (-> 255.0) in block 0; msdire in {-1, 0, 1}
    msdire[0, 1, 2, 3] = 2                          # one direction label outside that set: w = 4 + M
    msdire[n - 1, 2, 15, 15] = -3
    msbt[0, :, 1, 1] = 0
    msdire[0, :, 1, 1] = 0
    rng = np.random.default_rng(seed + 1)
    ql, bl, dl = V.loader_labels(qt8, msbt, msdire)
    qt = (ql + rng.normal(0, 0.45, ql.shape)).astype(np.float32)
    bt = (bl + rng.normal(0, 0.45, bl.shape)).astype(np.float32)
    dire = (dl + rng.normal(0, 0.45, dl.shape)).astype(np.float32)
    # logits exactly equal to their labels: zero terms, zero gradients
    qt[:, 0, 1:4] = ql[:, 0, 1:4]
    qt[0, 0, 0] = ql[0, 0, 0]                       # the 255.0 of a raw 0
    bt[:, :, 0, 0:3] = bl[:, :, 0, 0:3]
    dire[:, :, 0, 2:5] = dl[:, :, 0, 2:5]
    bt[:, 1, 3, 3] = bl[:, 1, 3, 3]                 # one layer only: the plain term is zero, the layer differences are not
    # -0.0 logits against a label of 0
    bt[0, :, 1, 1] = -0.0
    dire[0, :, 1, 1] = -0.0
    # layer differences that cancel exactly in float32 while the plain terms do not: the same dyadic offset on neighbouring layers
    bt[:, 0, 2, 4:8] = bl[:, 0, 2, 4:8] + np.float32(0.25)
    bt[:, 1, 2, 4:8] = bl[:, 1, 2, 4:8] + np.float32(0.25)
    bt[:, 1, 4, 0:4] = bl[:, 1, 4, 0:4] - np.float32(0.5)
    bt[:, 2, 4, 0:4] = bl[:, 2, 4, 0:4] - np.float32(0.5)
    if nonfinite:
        b = n - 1
        qt[b, 1, 2], qt[b, 1, 3], qt[0, 2, 2] = np.nan, np.inf, -np.inf
        bt[b, 0, 5, 6], bt[b, 2, 5, 7], bt[0, 1, 5, 8] = np.nan, np.inf, -np.inf
        bt[b, 0, 6, 6] = bt[b, 1, 6, 6] = np.inf    # inf - inf in the layer difference of k = 1
        bt[0, 1, 6, 9] = bt[0, 2, 6, 9] = -np.inf   # ... and of k = 2
        dire[b, 1, 5, 6], dire[b, 2, 7, 8], dire[0, 0, 9, 9] = -np.inf, np.nan, np.inf
    return {"comp": comp, "qp": qp, "n": n, "lam": dict(lam), "passes": passes, "qt": qt, "bt": bt, "dire": dire, "qt8": qt8, "msbt": msbt,
            "msdire": msdire}


def kw_of(c, mode="qbd", s=slice(None)):
    kw = {}
    if mode in ("qbd", "q"):
        kw.update(qt=c["qt"][s], qt8=c["qt8"][s])
    if mode in ("qbd", "bd"):
        kw.update(bt=c["bt"][s], dire=c["dire"][s], msbt=c["msbt"][s], msdire=c["msdire"][s])
    return kw


def lam_of(c, mode):
    """The case's weights; pre_train_Q's L1 has none, so the "q" form is called with lambq = 1 (include/pmp.h)."""
    lam = dict(c["lam"])
    if mode == "q":
        lam["lambq"] = 1.0
    return lam


def weights(comp, qp, dl):
    """w_k f32[n,16,16]: dl_k*dl_k + float32(M[int((qp - 22) / 5)][k]), M by component; w_0 = 1.0 when qp == 22."""
    row = (LUMA_MAT if comp == "Luma" else CHROMA_MAT)[int((qp - 22) / 5)]
    w = [dl[:, k] * dl[:, k] + np.float32(row[k]) for k in range(3)]
    if qp == 22:
        w[0] = np.ones_like(w[0])
    return w


def _terms32(comp, qp, qt=None, bt=None, dire=None, qt8=None, msbt=None, msdire=None):
    """The float32 terms BEFORE abs, as the sums and the signs see them: {"q": [n,8,8], "b"/"d"/"wd"/"wb": 3 x [n,16,16], "w": 3 x [n,16,16]}."""
    t = {}
    with np.errstate(invalid="ignore", over="ignore"):
        if qt is not None:
            t["q"] = qt.reshape(-1, 8, 8).astype(np.float32) - (qt8.reshape(-1, 8, 8) - np.uint8(1)).astype(np.float32)
        if bt is not None:
            bl, dl = msbt.astype(np.float32), msdire.astype(np.float32)
            w = weights(comp, qp, dl)
            t["w"] = w
            t["b"] = [bt[:, k] - bl[:, k] for k in range(3)]
            t["d"] = [dire[:, k] - dl[:, k] for k in range(3)]
            t["wd"] = [w[k] * dire[:, k] - w[k] * dl[:, k] for k in range(3)]
            t["wb"] = [w[0] * bt[:, 0] - w[0] * bl[:, 0]] + [w[k] * (bt[:, k] - bt[:, k - 1]) - w[k] * (bl[:, k] - bl[:, k - 1]) for k in (1, 2)]
    return t


def _wave(v):
    """The __shfl_xor butterfly over 64 lane partials f64[n,64] (offsets 32, 16, .. 1) as lane 0 ends up with it."""
    for h in (32, 16, 8, 4, 2, 1):
        v = v[:, :h] + v[:, h:2 * h]
    return v[:, 0]


def _map_sum(t):
    """One 16x16 map of float32 terms per block -> f64[n]: lane l adds |cells 4l..4l+3| in order, then the butterfly."""
    c = np.abs(t).reshape(len(t), 64, 4).astype(np.float64)
    return _wave(((c[..., 0] + c[..., 1]) + c[..., 2]) + c[..., 3])


def block_terms(comp, qp, **kw):
    """The thirteen sums per block, float64[n,13], with the kernel's order of additions."""
    t = _terms32(comp, qp, **kw)
    n = len(t["q"]) if "q" in t else len(t["b"][0])
    P = np.zeros((n, NTERMS), np.float64)
    with np.errstate(invalid="ignore"):
        if "q" in t:
            P[:, 0] = _wave(np.abs(t["q"]).reshape(n, 64).astype(np.float64))
        if "b" in t:
            for k in range(3):
                P[:, 1 + k], P[:, 4 + k], P[:, 7 + k], P[:, 10 + k] = _map_sum(t["b"][k]), _map_sum(t["d"][k]), _map_sum(t["wd"][k]), _map_sum(t["wb"][k])
    return P


def reduce_blocks(P):
    """sum_rows_kernel's order (logitstats.hip): row group g adds rows g, g + 16, .. in order, then the 16 group partials are added in order."""
    acc = np.zeros((16, NTERMS), np.float64)
    with np.errstate(invalid="ignore"):
        for r in range(len(P)):
            acc[r % 16] += P[r]
        tot = acc[0].copy()
        for g in range(1, 16):
            tot += acc[g]
    return tot


def terms(comp, qp, passes=None, **kw):
    """T[0..12] of one call.  passes: the block counts of the host form's passes - the pass sums added in pass order."""
    if passes is None:
        return reduce_blocks(block_terms(comp, qp, **kw))
    T = np.zeros(NTERMS, np.float64)
    o = 0
    with np.errstate(invalid="ignore"):
        for m in passes:
            T += reduce_blocks(block_terms(comp, qp, **{k: a[o:o + m] for k, a in kw.items()}))
            o += m
    return T


def loss_value(T, lam, n):
    """lambq*T0/(64n) + (lambb0*T1 + ... + lambresb2*T12)/(256n), float64, in that order."""
    T = [np.float64(x) for x in T]
    L = {k: np.float64(lam[k]) for k in KEYS}
    d64, d256 = np.float64(64 * n), np.float64(256 * n)
    with np.errstate(invalid="ignore", over="ignore"):
        return L["lambq"] * T[0] / d64 + (L["lambb0"] * T[1] + L["lambb1"] * T[2] + L["lambb2"] * T[3] + L["lambd0"] * T[7] + L["lambd1"] * T[8]
                                         + L["lambd2"] * T[9] + L["lambresb0"] * T[10] + L["lambresb1"] * T[11] + L["lambresb2"] * T[12]) / d256


def _sgn(t):
    """torch.sign as float64: +1, -1, and +0.0 for zeros of either sign and for NaN."""
    return (t > 0).astype(np.float64) - (t < 0).astype(np.float64)


def grads(comp, qp, lam, n_div, **kw):
    """{"qt": f32[n,8,8], "bt": f32[n,3,16,16], "dire": f32[n,3,16,16]} for the logits given: float64 arithmetic from the float32 w and
    the signs of the float32 terms, left to right as the header writes it, rounded once.  n_div: the n of the divisors."""
    t = _terms32(comp, qp, **kw)
    L = {k: np.float64(lam[k]) for k in KEYS}
    d64, d256 = np.float64(64 * n_div), np.float64(256 * n_div)
    g = {}
    with np.errstate(invalid="ignore"):
        if "q" in t:
            g["qt"] = (L["lambq"] * _sgn(t["q"]) / d64).astype(np.float32)
        if "b" in t:
            w = [x.astype(np.float64) for x in t["w"]]
            a, c, e = [_sgn(x) for x in t["b"]], [_sgn(x) for x in t["wd"]], [_sgn(x) for x in t["wb"]]
            gb, gd = [], []
            for k in range(3):
                gd.append((L["lambd%d" % k] * w[k] * c[k] / d256).astype(np.float32))
                v = L["lambb%d" % k] * a[k] + L["lambresb%d" % k] * w[k] * e[k]
                if k < 2:
                    v = v - L["lambresb%d" % (k + 1)] * w[k + 1] * e[k + 1]
                gb.append((v / d256).astype(np.float32))
            g["bt"], g["dire"] = np.stack(gb, axis=1), np.stack(gd, axis=1)
    return g


def same_bits(a, b):
    """Equal bit for bit; a NaN equals a NaN (its sign and payload are nobody's contract)."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    u = {4: np.uint32, 8: np.uint64}[a.dtype.itemsize]
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(a.view(u)[~na], b.view(u)[~nb]))


def grad_dist(ref, mine):
    """Largest |ref - mine| / max |ref| of one gradient tensor (0 for an all-zero reference that mine equals)."""
    ref, mine = np.asarray(ref, np.float64), np.asarray(mine, np.float64)
    den = np.max(np.abs(ref))
    d = np.max(np.abs(ref - mine))
    return 0.0 if d == 0 else float(d / den)


def same_zero_nan_pattern(ref, mine):
    return bool(np.array_equal(ref == 0, mine == 0) and np.array_equal(np.isnan(ref), np.isnan(mine)))
