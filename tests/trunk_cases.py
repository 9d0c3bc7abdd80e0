"""Cases and a float64 restatement of a TRUNK of Model_QBD.ResidualBlocks with an optional 2x2 max-pool, forward and backward
(include/pmp.h: pmp_trunk_*; csrc/api_train.cpp, trunk_glue.hip).  Shared by tests/test_trunk_cases_cpu.py,
tests/test_gpu_trunk_grad.py and tools/gen_golden_trunk.py.  The blocks are resblock_cases.forward / backward chained; the pool and its
backward are written out here with the first-maximum rule, not taken from autograd.

EXACT cases.  x uniform integers in [-2, 2], the upstream gradient in {-1, 0, 1}, weights SPARSE +-1: a tap is nonzero with probability
5 / fan-in, a shortcut weight with probability 2 / cin.  (Dense +-1 weights, as in resblock_cases, leave float32's exact integers
behind two blocks; these do not.)  worst_partial_sum() chains resblock_cases.worst_partial_sum over the blocks, each on the
magnitudes of its actual inputs: below 2^24 on every case (tests/test_trunk_cases_cpu.py), so float32 in ANY order equals float64 bit
for bit, no element left out.  The outputs are small integers, so the pooled cases have windows whose positive maximum occurs more than
once: the tie rule is exercised (tied_positive_windows()).

FLOAT cases.  Normal values, weights scaled by 1 / sqrt(fan-in): for comparing the trunk call with the chain of block calls, which
run the same kernels in the same order.
"""
import os

import numpy as np
import torch

import resblock_cases as K

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g16_trunk_grad.npz")

# name -> (n, h, w, cin, [(cout, k), ...], pool)
EXACT = {
    "one_pool": (2, 16, 16, 16, [(16, 3)], 1),                        # one block and a pool
    "m2_like":  (2, 32, 32, 64, [(64, 3)] * 3, 1),                    # identity-shortcut chain, tile halos
    "m1_like":  (2, 32, 32, 32, [(64, 5), (64, 3)], 1),               # mixed k, a shortcut then an identity
    "b_like":   (3, 16, 16, 64, [(32, 3), (16, 3), (8, 3)], 0),       # narrowing, padded channels, odd n
    "b3_like":  (2, 32, 32, 64, [(32, 3), (16, 3), (8, 3)], 1),       # pool on a padded 8-channel group
    "att_like": (2, 16, 48, 3, [(32, 3), (64, 3)], 0),                # padded cin, non-square
    "six":      (5, 16, 16, 16, [(16, 3)] * 6, 1),                    # trunk_M1's length
}
IN_GOLDEN = ("one_pool", "m1_like", "b_like")
FLOAT = {"f_m1_like": EXACT["m1_like"], "f_b3_like": EXACT["b3_like"], "f_m2_like": EXACT["m2_like"]}


def _seed(name):
    return 20232 + sum((i + 1) * ord(ch) for i, ch in enumerate(name))


def block_shapes(shape):
    """-> [(cin_i, cout_i, k_i), ...]"""
    cins = [shape[3]] + [c for c, _ in shape[4][:-1]]
    return [(ci, co, k) for ci, (co, k) in zip(cins, shape[4])]


def y_shape(shape):
    n, h, w, _, blocks, pool = shape
    return (n, blocks[-1][0], h // 2, w // 2) if pool else (n, blocks[-1][0], h, w)


def make_case(shape, seed, exact=True):
    """A trunk of `shape` from `seed` -> dict(shape, x, blocks [(w0, w2, wsc or None), ...], g_y) as float32 numpy arrays: the EXACT scheme
    (small integers, sparse +-1 weights) or, with exact=False, the FLOAT one (normal values, weights scaled by 1 / sqrt(fan-in))."""
    n, h, w, cin = shape[:4]
    g = torch.Generator().manual_seed(seed)
    ri = lambda lo, hi, *s: torch.randint(lo, hi + 1, s, generator=g).to(torch.float32).numpy()
    rn = lambda scale, *s: (torch.randn(s, generator=g, dtype=torch.float64) * scale).to(torch.float32).numpy()

    def sparse(p, *s):                              # +-1 with probability p (capped at 1), else 0
        on = (torch.rand(s, generator=g) < p).to(torch.float32).numpy()
        return on * (2 * ri(0, 1, *s) - 1)

    c = {"shape": shape, "x": ri(-2, 2, n, cin, h, w) if exact else rn(1.0, n, cin, h, w), "blocks": []}
    for ci, co, k in block_shapes(shape):
        if exact:
            c["blocks"].append((sparse(5.0 / (ci * k * k), co, ci, k, k), sparse(5.0 / (co * k * k), co, co, k, k),
                                sparse(2.0 / ci, co, ci) if ci != co else None))
        else:
            c["blocks"].append((rn((ci * k * k) ** -0.5, co, ci, k, k), rn((co * k * k) ** -0.5, co, co, k, k),
                                rn(ci ** -0.5, co, ci) if ci != co else None))
    c["g_y"] = ri(-1, 1, *y_shape(shape)) if exact else rn(1.0, *y_shape(shape))
    return c


def make_exact(name):
    """-> dict(shape, x, blocks [(w0, w2, wsc or None), ...], g_y) as float32 numpy arrays of small integers."""
    return make_case(EXACT[name], _seed(name), True)


def make_float(name):
    """-> the same with normal values; weights scaled by 1 / sqrt(fan-in)."""
    return make_case(FLOAT[name], _seed(name), False)


def _windows(a):
    """[n, c, h, w] -> [n, c, h/2, w/2, 4]: the elements of every 2x2 window in the order (0,0), (0,1), (1,0), (1,1)."""
    return np.stack([a[:, :, 0::2, 0::2], a[:, :, 0::2, 1::2], a[:, :, 1::2, 0::2], a[:, :, 1::2, 1::2]], axis=-1)


def pool(a):
    return _windows(a).max(axis=-1)


def pool_backward(a, g):
    """The gradient g of pool(a) handed to the FIRST maximum of every window (np.argmax returns the first), zero elsewhere."""
    first = _windows(a).argmax(axis=-1)
    r = np.zeros(a.shape, g.dtype)
    for e in range(4):
        r[:, :, e >> 1::2, e & 1::2] = np.where(first == e, g, 0)
    return r


def tied_positive_windows(a):
    """How many 2x2 windows of a hold their maximum more than once, the maximum being positive."""
    w = _windows(a)
    m = w.max(axis=-1, keepdims=True)
    return int((((w == m).sum(axis=-1) > 1) & (m[..., 0] > 0)).sum())


def restate(c, dtype=torch.float64, want_g_x=True):
    """Forward and backward of a case -> dict(y, t [per block], out [per block, un-pooled], g_x, g_w [(g_w0, g_w2, g_wsc or None) per
    block], g_out [per block: the upstream gradient that reached it]) as numpy arrays of `dtype`."""
    np_dtype = np.float64 if dtype == torch.float64 else np.float32
    x = np.asarray(c["x"], np_dtype)
    r = {"t": [], "out": [], "g_w": [None] * len(c["blocks"]), "g_out": [None] * len(c["blocks"]), "g_x": None}
    for w0, w2, wsc in c["blocks"]:
        t, out = K.forward(x, w0, w2, wsc, dtype)
        r["t"].append(t)
        r["out"].append(out)
        x = out
    pooled = c["shape"][5]
    r["y"] = pool(x) if pooled else x
    g = np.asarray(c["g_y"], np_dtype)
    if pooled:
        g = pool_backward(r["out"][-1], g)
    for i in range(len(c["blocks"]) - 1, -1, -1):
        w0, w2, wsc = c["blocks"][i]
        b = K.backward(c["x"] if i == 0 else r["out"][i - 1], r["t"][i], r["out"][i], w0, w2, wsc, g, dtype, want_g_x=want_g_x or i > 0)
        r["g_out"][i] = g
        r["g_w"][i] = (b["g_w0"], b["g_w2"], b["g_wsc"])
        g = b["g_x"]
    r["g_x"] = g
    return r


def worst_partial_sum(c):
    """resblock_cases.worst_partial_sum of every block on its actual inputs (its x, and the upstream gradient that reached it), the
    largest of them: a bound on every partial sum any kernel of the trunk can form, whatever its order.  The pool adds nothing."""
    r = restate(c)
    worst = 0.0
    for i, (w0, w2, wsc) in enumerate(c["blocks"]):
        b = {"x": c["x"] if i == 0 else r["out"][i - 1], "w0": w0, "w2": w2, "wsc": wsc, "g_out": r["g_out"][i]}
        worst = max(worst, K.worst_partial_sum(b))
    return worst


def flat(r):
    """A restatement (or a kernel's results laid out like one) as a flat dict name -> array: y, g_x, t<i>, out<i>, g_w0_<i>, ..."""
    d = {"y": r["y"], "g_x": r["g_x"]}
    for i in range(len(r["t"])):
        d["t%d" % i], d["out%d" % i] = r["t"][i], r["out"][i]
        for nm, a in zip(("g_w0", "g_w2", "g_wsc"), r["g_w"][i]):
            if a is not None:
                d["%s_%d" % (nm, i)] = a
    return {k: v for k, v in d.items() if v is not None}


def golden_keys(d):
    """The names of flat(d) the golden stores: the calls' outputs; the saved tensors are checked when it is generated."""
    return [k for k in d if k in ("y", "g_x") or k.startswith("g_w")]
