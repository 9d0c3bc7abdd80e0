"""Cases and a float64 restatement of a QT net's TAIL, forward and backward (include/pmp.h: pmp_qtail_*; csrc/api_train.cpp,
qtail_train.hip): resblock_q3, the multi-scale pool, resblock_q4, resblock_q5 with its 2x2 pool, resblock_q6.  Shared by
tests/test_qtail_cases_cpu.py, tests/test_gpu_qtail_grad.py and tools/gen_golden_qtail.py.  The blocks are resblock_cases.forward /
backward, q5's pool trunk_cases'; the multi-scale pool and its backward are written out here from include/pmp.h's formulas - the first
maximum of the WHOLE window in row-major order, the window's sum added element by element - not taken from autograd.

EXACT cases, name -> (n, h, w).  x4 uniform integers in [-2, 2], g_x9 in {-1, 0, 1}, trunk_cases' sparse +-1 weights.
worst_partial_sum() stays below 2^24 on every one (tests/test_qtail_cases_cpu.py), so float32 in ANY order equals float64 bit for bit.
The activations are small integers, so windows whose positive maximum occurs more than once are plentiful at every scale
(tied_positive()), and a backward pass that took the argmax of a hierarchy of 2x2 maxima would give another g_x4 (restate(c,
hierarchical=True)).
  nets (1, 16, 16)      the nets' own shape: one tile, q6's 8x8 map in a corner of one
  tall (3, 32, 16)      two tiles in a column, 6 work items of the weight gradients' reduction at full size and 3 on q6's map
  wide (2, 16, 48)      three tiles in a row, q6's 8 x 24 map in a 16 x 32 one: 6 items and 4
  five (5, 16, 16)      an odd partition: 5 items, NP = 3
FLOAT cases, name -> ((n, h, w), kind) with grad_cases' kinds `randn` and `positive`, weights normal / sqrt(fan-in).

BOUND of the float cases (tests/test_gpu_qtail_grad.py), grad_cases' form per element:
    |gpu - ref64| <= c * 2^-24 * A + 2^-23 * |ref64| + P
Every tensor is made by conv_mfma (c = C_CONV = 24; q4's chain of 128 * 9 + 128 = 1280 terms is below the 1664 it was derived for) or by
wgrad_partial_kernel (c = C_WGRAD = 33; the longest chain of one workgroup in the float cases is 512 pixels, within the 768 it was
derived on: longest_wgrad_chain()).  No new kernel multiplies or adds products: q6 runs through the same two kernels on its map.
So that a ReLU mask or a pool's argmax that a rounding error flips cannot enter, every operation is checked LOCALLY: the float64
reference of a block is evaluated on the inputs, masks and maxima the GPU itself saved (pmp_qtail_unpack_device), and the error a
gradient already carries when it reaches an operation is pushed through that operation's absolute-value companion (P).
Constants: C_CONV = 24, C_WGRAD = 33 (grad_cases'), and 66 units of 2^-24 * A for the multi-scale pool's backward (at most 63 + 3
float32 additions per element).  Largest |gpu - ref64| / bound measured on an MI355X (printed by the test under `pytest -s`): 0.301
on the convolutions (q3's t, f_positive_32x32), 0.336 on the weight gradients (q6's g_w2, f_positive_32x32), below 0.001 on g_x4.
"""
import functools
import os

import numpy as np
import torch

import resblock_cases as K
import trunk_cases as T

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g20_qtail_grad.npz")

BLOCKS = ((64, 32, 3), (128, 32, 3), (32, 32, 3), (32, 8, 3))          # (cin, cout, k) of q3, q4, q5, q6
EXACT = {"nets": (1, 16, 16), "tall": (3, 32, 16), "wide": (2, 16, 48), "five": (5, 16, 16)}
FLOAT = {"f_%s_%dx%d" % (kind, s[1], s[2]): (s, kind) for s in ((2, 16, 16), (1, 32, 32)) for kind in ("randn", "positive")}
SCALES = (2, 4, 8)


def _seed(name):
    return 20240 + sum((i + 1) * ord(ch) for i, ch in enumerate(name))


def make_case(shape, seed, kind="exact"):
    """-> dict(shape, x4, blocks [(w0, w2, wsc or None)] * 4, g_x9) as float32 numpy arrays."""
    n, h, w = shape
    g = torch.Generator().manual_seed(seed)
    ri = lambda lo, hi, *s: torch.randint(lo, hi + 1, s, generator=g).to(torch.float32).numpy()
    rn = lambda scale, *s: (torch.randn(s, generator=g, dtype=torch.float64) * scale).to(torch.float32).numpy()
    logu = lambda lo, hi, *s: (2.0 ** (lo + (hi - lo) * torch.rand(s, generator=g, dtype=torch.float64))).to(torch.float32).numpy()

    def sparse(p, *s):                              # +-1 with probability p (capped at 1), else 0
        on = (torch.rand(s, generator=g) < p).to(torch.float32).numpy()
        return on * (2 * ri(0, 1, *s) - 1)

    sx, sg = (n, 64, h, w), (n, 8, h // 2, w // 2)
    c = {"shape": shape, "blocks": []}
    if kind == "exact":
        c["x4"], c["g_x9"] = ri(-2, 2, *sx), ri(-1, 1, *sg)
    elif kind == "randn":
        c["x4"], c["g_x9"] = rn(1.0, *sx), rn(1.0, *sg)
    elif kind == "positive":
        c["x4"], c["g_x9"] = logu(-6, 6, *sx), logu(-6, 6, *sg)
    else:
        raise KeyError(kind)
    for ci, co, k in BLOCKS:
        if kind == "exact":
            c["blocks"].append((sparse(5.0 / (ci * k * k), co, ci, k, k), sparse(5.0 / (co * k * k), co, co, k, k),
                                sparse(2.0 / ci, co, ci) if ci != co else None))
        else:
            c["blocks"].append((rn((ci * k * k) ** -0.5, co, ci, k, k), rn((co * k * k) ** -0.5, co, co, k, k),
                                rn(ci ** -0.5, co, ci) if ci != co else None))
    return c


def make_exact(name):
    return make_case(EXACT[name], _seed(name))


def make_float(name):
    shape, kind = FLOAT[name]
    return make_case(shape, _seed(name), kind)


# ---- the multi-scale pool (include/pmp.h)
def _win(a, s):
    """[n, c, h, w] -> [n, c, h/s, w/s, s*s]: every s x s window, its elements in row-major order."""
    n, c, h, w = a.shape
    return a.reshape(n, c, h // s, s, w // s, s).transpose(0, 1, 2, 4, 3, 5).reshape(n, c, h // s, w // s, s * s)


def _unwin(a, s):
    n, c, hs, ws, _ = a.shape
    return a.reshape(n, c, hs, ws, s, s).transpose(0, 1, 2, 4, 3, 5).reshape(n, c, hs * s, ws * s)


def multipool(x5):
    """x6 = cat[x5, up2(mp2(x5)), up4(mp4(x5)), up8(mp8(x5))]"""
    parts = [x5]
    for s in SCALES:
        m = _win(x5, s).max(axis=-1, keepdims=True)
        parts.append(_unwin(np.broadcast_to(m, m.shape[:-1] + (s * s,)), s))
    return np.concatenate(parts, axis=1)


def _hier_first(win, s):
    """The argmax of a hierarchy of 2x2 maxima of [..., s, s] windows -> (max, index in row-major order): NOT the tail's rule."""
    if s == 1:
        return win[..., 0, 0], np.zeros(win.shape[:-2], np.int64)
    hs = s // 2
    quads = [_hier_first(win[..., qy * hs:(qy + 1) * hs, qx * hs:(qx + 1) * hs], hs) for qy in (0, 1) for qx in (0, 1)]
    m = np.stack([q[0] for q in quads], axis=-1)
    first = m.argmax(axis=-1)
    idx = np.zeros(first.shape, np.int64)
    for e, (_, sub) in enumerate(quads):
        full = ((e >> 1) * hs + sub // hs) * s + (e & 1) * hs + sub % hs
        idx = np.where(first == e, full, idx)
    return m.max(axis=-1), idx


def multipool_backward(x5, g6, hierarchical=False):
    """g_x5 from g6 [n, 128, h, w], in g6's dtype: g = g6[c]; g = g + r2; g = g + r4; g = g + r8.  r_s: the window's sum of
    g6[32 log2(s) + c], from +0 in row-major order, at the first maximum of the whole window in row-major order; +0 elsewhere."""
    g = g6[:, 0:32].copy()
    for ls, s in enumerate(SCALES, 1):
        xw, gw = _win(x5, s), _win(g6[:, 32 * ls:32 * ls + 32], s)
        if hierarchical:
            first = _hier_first(xw.reshape(xw.shape[:-1] + (s, s)), s)[1]
        else:
            first = xw.argmax(axis=-1)                                  # numpy returns the first of equal maxima
        acc = np.zeros(gw.shape[:-1], g6.dtype)
        for e in range(s * s):
            acc = acc + gw[..., e]
        r = np.where(np.arange(s * s) == first[..., None], acc[..., None], np.zeros((), g6.dtype))
        g = g + _unwin(r, s)
    return g


def tied_positive(a, s):
    """How many s x s windows of a hold their maximum more than once, the maximum being positive."""
    w = _win(a, s)
    m = w.max(axis=-1, keepdims=True)
    return int((((w == m).sum(axis=-1) > 1) & (m[..., 0] > 0)).sum())


# ---- the whole tail
def restate(c, dtype=torch.float64, want_g_x=True, hierarchical=False):
    """Forward and backward of a case -> dict(x9, g_x4, s [the nine saved tensors of pmp_qtail_unpack_device], g_w [(g_w0, g_w2, g_wsc
    or None) per block], x6, x8, g_in [per block: its input], g_out [per block: the upstream gradient that reached it], g6) as numpy
    arrays of `dtype`."""
    npd = np.float64 if dtype == torch.float64 else np.float32
    x4 = np.asarray(c["x4"], npd)
    b = c["blocks"]
    t3, x5 = K.forward(x4, *b[0], dtype)
    x6 = multipool(x5)
    t4, x7 = K.forward(x6, *b[1], dtype)
    t5, o5 = K.forward(x7, *b[2], dtype)
    x8 = T.pool(o5)
    t6, x9 = K.forward(x8, *b[3], dtype)
    r = {"x9": x9, "s": [x4, t3, x5, t4, x7, t5, o5, t6, x9], "x6": x6, "x8": x8, "g_w": [None] * 4, "g_out": [None] * 4,
         "g_in": [x4, x6, x7, x8]}
    g = np.asarray(c["g_x9"], npd)
    ins, ts, outs = r["g_in"], [t3, t4, t5, t6], [x5, x7, o5, x9]
    for i in (3, 2, 1, 0):
        r["g_out"][i] = g
        bk = K.backward(ins[i], ts[i], outs[i], *b[i], g, dtype, want_g_x=want_g_x or i > 0)
        r["g_w"][i] = (bk["g_w0"], bk["g_w2"], bk["g_wsc"])
        g = bk["g_x"]
        if i == 3:
            g = T.pool_backward(o5, g)
        if i == 1:
            r["g6"] = g
            g = multipool_backward(x5, g, hierarchical)
    r["g_x4"] = g
    return r


def worst_partial_sum(c):
    """The largest sum of |terms| any kernel of the tail can form: resblock_cases.worst_partial_sum of every block on its actual inputs,
    and the multi-scale pool's backward (at most 1 + 4 + 16 + 64 terms per element)."""
    r = restate(c)
    worst = 0.0
    for i, (w0, w2, wsc) in enumerate(c["blocks"]):
        worst = max(worst, K.worst_partial_sum({"x": r["g_in"][i], "w0": w0, "w2": w2, "wsc": wsc, "g_out": r["g_out"][i]}))
    g6 = np.abs(r["g6"])
    pool = g6[:, 0:32].max() + sum(_win(g6[:, 32 * ls:32 * ls + 32], s).sum(axis=-1).max() for ls, s in enumerate(SCALES, 1))
    return max(worst, float(pool))


def flat(r):
    """A restatement (or the calls' results laid out like one) as a flat dict name -> array: x9, g_x4, s0 .. s8, g_w0_<i>, ..."""
    d = {"x9": r["x9"], "g_x4": r["g_x4"]}
    for i, a in enumerate(r["s"]):
        d["s%d" % i] = a
    for i in range(4):
        for nm, a in zip(("g_w0", "g_w2", "g_wsc"), r["g_w"][i]):
            if a is not None:
                d["%s_%d" % (nm, i)] = a
    return {k: v for k, v in d.items() if v is not None}


def golden_keys(d):
    """The names of flat(d) the golden stores: the calls' outputs; the saved tensors are checked when it is generated."""
    return [k for k in d if k in ("x9", "g_x4") or k.startswith("g_w")]


@functools.lru_cache(maxsize=None)
def exact(name):
    """-> (case, flat float64 restatement); computed once, never changed."""
    c = make_exact(name)
    return c, flat(restate(c))


def longest_wgrad_chain(shape):
    """The most pixels one workgroup of wgrad_partial_kernel adds in a tail of this shape: ceil(items / NP) tiles of 256, at full
    size with Ca = 32, 64 and 128 and on q6's map."""
    n, h, w = shape
    h2, w2 = (h // 2 + 15) // 16 * 16, (w // 2 + 15) // 16 * 16
    worst = 0
    for hh, ww, cas in ((h, w, (32, 64, 128)), (h2, w2, (16, 32))):
        for ca in cas:
            items = n * (hh // 16) * (ww // 16)
            np_ = min((items + 1) // 2, 256 // (ca // 16))
            worst = max(worst, -(-items // np_) * 256)
    return worst
