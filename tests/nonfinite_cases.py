"""NaN and inf through the training calls (include/pmp.h: NON-FINITE VALUES IN THE TRAINING CALLS): cases and CPU machinery only, shared
by tests/test_nonfinite_cases_cpu.py and tests/test_gpu_nonfinite.py.  Shapes, values and weights come from the case modules of the calls
(trunk_cases.make_case - a ResidualBlock is a trunk of one block without a pool -, qtail_cases.make_case, stem_cases.make_case); nothing
of them is restated here.

What IS new here is the reference: the calls as torch ops UNDER AUTOGRAD (F.conv2d, F.relu, F.max_pool2d, F.interpolate as Model_QBD.py
uses them), because the case modules' written-out backward passes - where(x > 0, g, 0), the first maximum of a window - are deliberately
not autograd's and turn a NaN mask into zeros, which torch's threshold_backward and max_pool2d's backward do not.

A net is written ONCE, over an `ops` object (block_net, trunk_net, qtail_net, stem_net), and runs in two modes:
  Real        torch ops on float64 or float32 tensors; reference(case, dtype) runs it under autograd -> every tensor the call writes.
              R, the footprint a call must DETECT, is where that result is not finite (footprints()).
  Indicator   the reach S, which a call must stay INSIDE: every weight is one (all channels connected), a ReLU passes everything, the
              pools are kept; forward on the 0/1 indicator of the planted input elements; backward on the indicator of the planted
              gradient elements, OR'ed at every ReLU and every pool with the forward indicator of what the gradient is masked by there
              (a pool: by the whole window).  Non-zero = reachable.  Weight and bias gradients are wholly reachable, and with a plant in a
              weight or a bias so is everything.  reach(case) -> the same names as reference().
Outside S a result does not depend on the plant at all: it is what the call gives on the clean case (clean(case)).

CASES.  family/shape/plant.  Every shape has n = 2 and every plant lies in image 0, so S never covers more than half of a data tensor.
Values are the `randn` scheme of the case modules: normal data, weights normal / sqrt(fan-in).
  nan_corner  NaN at (0, 0) of channel 0                       nan_seam   NaN at (15, 15), where four 16x16 tiles meet or a map ends,
  pinf, ninf  +inf / -inf at an interior pixel                            in channel 1 (channel 0 of a one-channel stem)
  pair        +inf and -inf one pixel apart in one channel: the NaN is born inside the first convolution
  pool_last   NaN at (7, 7), the last element of its 2x2, 4x4 and 8x8 window (the shapes with a pool)
  g           NaN in the upstream gradient where the output is positive (_g_index), clean data
  w0, w2, wsc, b   NaN in a weight (output 0, input 0, the centre tap; a stem: tap (0, 0), which is its own pixel's) or in bias 0; a
                   chain: w0 of the first block, w2 of the last (the QT tail: of q4), the first shortcut
  overflow    the inf is born by float32 overflow: two inputs of 3e38 side by side in one channel.  So that EVERY order of summation
              overflows at the same elements: the first convolution's weights (a stem's biases too) are |normal|, and WITHOUT the
              1 / sqrt(fan-in) - two products of 3e38 times a weight around 0.8 have to pass 3.4e38, which the scaled weights do not;
              every other input of a sum that holds a plant is +0 (non-negative, and the rest of the map keeps its signs: sums of
              hundreds of terms of ONE sign are not what grad_cases' bound was derived on); and the gradients' sums are kept free of
              an order too: behind a chain the upstream gradient of image 0 is +0 (every term is 0 times inf = NaN or 0 times 3e38 =
              0), behind a stem it is |normal| (the two large terms of a weight gradient have one sign).  Its mixed-sign twin - a
              weight gradient a * 3e38 - b * 3e38 - is finite on an MFMA, whose four-term inner product does not round to float32 in
              between, and inf in torch: no footprint either side must have.  float64 does not overflow: the reference footprint of
              this case alone is torch CPU float32.
HEADS and GATE: a table, reference and reach of their own at the end of this module (HEAD_CASES, head_reference, head_reach, gate_make).
STEM, split: the library runs ONE k x k convolution whose smaller kernels are zero-padded (csrc/stem_train.hip), and 0 * NaN = NaN: the
indicator run of a split stem uses that k x k kernel for all 32 outputs - all taps connected, as all channels are.
"""
import functools

import numpy as np
import torch
import torch.nn.functional as F

import qtail_cases as Q
import stem_cases as S
import trunk_cases as T

NAN, INF, BIG = float("nan"), float("inf"), 3e38

# family -> shapes, as the family's case module writes a shape
SHAPES = {
    "block": [(2, 16, 32, 3, ((17, 3),), 0), (2, 16, 32, 16, ((16, 3),), 0), (2, 16, 32, 33, ((40, 5),), 0)],
    "trunk": [(2, 32, 16, 15, ((33, 3), (63, 5)), 1), (2, 16, 32, 3, ((32, 3), (64, 3)), 0)],
    "qtail": [(2, 16, 16), (2, 32, 16)],
    "stem": [(2, 16, 32, 1, 9, 0), (2, 32, 16, 2, 9, 1), (2, 16, 32, 3, 5, 0), (2, 32, 32, 4, 5, 1)],
}
X_OF = {"block": "x", "trunk": "x", "qtail": "x4", "stem": "x"}
G_OF = {"block": "g_y", "trunk": "g_y", "qtail": "g_x9", "stem": "g_y"}
Y_OF = {"block": "y", "trunk": "y", "qtail": "x9", "stem": "y"}
# The QT tail's g plant, what find_g_at() finds (tests/test_nonfinite_cases_cpu.py holds the two together): from most elements of its 8x8
# or 16x8 output the NaN gradient runs along a map's border in some channel, where torch's float32 and float64 weight-gradient kernels
# disagree with each other (one multiplies the zero padding by the NaN, one skips it); from these it does not.
G_AT = {("qtail", (2, 16, 16)): (0, 0, 2, 4), ("qtail", (2, 32, 16)): (0, 0, 8, 4)}
DATA_PLANTS = ("nan_corner", "nan_seam", "pinf", "ninf", "pair", "pool_last", "overflow")     # in x: the forward pass sees them
WEIGHT_PLANTS = ("w0", "w2", "wsc", "b")


def has_pool(family, shape):
    return family == "qtail" or (family == "trunk" and bool(shape[5]))


def plants_of(family, shape):
    r = ["nan_corner", "nan_seam", "pinf", "ninf", "pair"] + (["pool_last"] if has_pool(family, shape) else []) + ["g"]
    if family == "stem":
        r += ["w0", "w2", "b"]                                      # w0: the first convolution's weight, w2: the last one's
    else:
        blocks = Q.BLOCKS if family == "qtail" else T.block_shapes(shape)
        r += ["w0", "w2"] + (["wsc"] if any(ci != co for ci, co, _ in blocks) else [])
    return r + ["overflow"]


def case_id(family, shape, plant):
    parts = ["_".join("%dk%d" % b for b in v) if isinstance(v, tuple) else str(v) for v in shape]
    return "%s-%s-%s" % (family, "x".join(parts), plant)


CASES = {case_id(f, s, p): (f, s, p) for f in SHAPES for s in SHAPES[f] for p in plants_of(f, s)}


def _seed(family, shape):
    return 20250 + sum((i + 1) * ord(ch) for i, ch in enumerate(case_id(family, shape, "")))


def _interior(shape):
    """(y, x) of the interior plants: no tile seam, no pool window's corner"""
    return shape[1] // 2 + 1, shape[2] // 2 - 3


def _first_k(family, shape):
    return shape[4] if family == "stem" else Q.BLOCKS[0][2] if family == "qtail" else shape[4][0][1]


def _weights(family, c):
    """-> [(name, array)] of every weight and bias of a case, by the names the plants use; the arrays are the case's own."""
    if family == "stem":
        return [("w%d" % j, a) for j, a in enumerate(c["w"])] + [("b%d" % j, a) for j, a in enumerate(c["b"])]
    return [("%s_%d" % (nm, i), a) for i, blk in enumerate(c["blocks"]) for nm, a in zip(("w0", "w2", "wsc"), blk) if a is not None]


@functools.lru_cache(maxsize=None)
def _clean(family, shape, overflow):
    if family == "stem":
        c = S.make_case(case_id(family, shape, ""), "randn", shape=shape)
    elif family == "qtail":
        c = Q.make_case(shape, _seed(family, shape), "randn")
    else:
        c = T.make_case(shape, _seed(family, shape), exact=False)
    if overflow:
        # the sums the overflow is born in: weights (and a stem's biases) |normal|, the weights' scaling undone; every other input of
        # a sum that holds a plant is +0; the upstream gradient of image 0 is +0 behind a chain (every gradient term there is then 0 times
        # something, the same in every order) and |normal| behind a stem (its weight gradients' two large terms have one sign)
        for nm, a in _weights(family, c):
            if nm == "w0_0" or family == "stem":
                a[...] = np.abs(a) * np.float32(np.sqrt(a[0].size) if nm.startswith("w") else 1)
        k = _first_k(family, shape)
        iy, ix = _interior(shape)
        c[X_OF[family]][0, :, iy - k + 1:iy + k, ix - k + 1:ix + 1 + k] = 0
        g = c[G_OF[family]]
        g[0] = np.abs(g[0]) if family == "stem" else 0
    return c


def _copy(c):
    d = dict(c)
    for k, v in c.items():
        if isinstance(v, np.ndarray):
            d[k] = v.copy()
        elif k == "blocks":
            d[k] = [tuple(None if a is None else a.copy() for a in blk) for blk in v]
        elif k in ("w", "b"):
            d[k] = [a.copy() for a in v]
    return d


def clean(name):
    """The case without its plants -> a fresh copy."""
    family, shape, plant = CASES[name]
    return dict(_copy(_clean(family, shape, plant == "overflow")), family=family)


@functools.lru_cache(maxsize=None)
def _g_index(family, shape):
    """Where the upstream gradient is planted: the first element of image 0, channel 1 from (3, 4) on whose output is positive - behind a
    ReLU that is off, torch too drops the gradient, and the case would test nothing."""
    if (family, shape) in G_AT:
        return G_AT[family, shape]
    y = reference(dict(_clean(family, shape, False), family=family))[Y_OF[family]][0, 1]
    at = np.flatnonzero(y.reshape(-1) > 0)
    return (0, 1) + tuple(int(v) for v in np.unravel_index(at[at >= 3 * y.shape[1] + 4][0], y.shape))


def find_g_at(family, shape):
    """The search behind G_AT: the first element of image 0 in row-major order (channel, y, x) whose output is positive and from which
    a NaN gradient leaves the same footprint in float32 and in float64."""
    base = dict(_clean(family, shape, False), family=family)
    y = reference(base)[Y_OF[family]]
    for idx in zip(*np.nonzero(y[0] > 0)):
        c = dict(_copy(base), family=family)
        c[G_OF[family]][(0,) + idx] = NAN
        a, b = footprints(reference(c, torch.float64)), footprints(reference(c, torch.float32))
        if all(np.array_equal(a[k], b[k]) for k in a):
            return (0,) + tuple(int(v) for v in idx)
    return None


def plants(name):
    """-> [(tensor name, index, value)]: tensor names are the case's x and g keys, and w0_<i> / w2_<i> / wsc_<i> (stem: w<j>, b<j>)."""
    family, shape, plant = CASES[name]
    c = _clean(family, shape, False)
    x, g = X_OF[family], G_OF[family]
    ch = 1 if c[x].shape[1] > 1 else 0
    iy, ix = _interior(shape)
    if plant == "nan_corner":
        return [(x, (0, 0, 0, 0), NAN)]
    if plant == "nan_seam":
        return [(x, (0, ch, 15, 15), NAN)]
    if plant in ("pinf", "ninf"):
        return [(x, (0, ch, iy, ix), INF if plant == "pinf" else -INF)]
    if plant == "pair":
        return [(x, (0, ch, iy, ix), INF), (x, (0, ch, iy, ix + 1), -INF)]
    if plant == "pool_last":
        return [(x, (0, ch, 7, 7), NAN)]
    if plant == "overflow":
        return [(x, (0, ch, iy, ix), BIG), (x, (0, ch, iy, ix + 1), BIG)]
    if plant == "g":
        return [(g, _g_index(family, shape), NAN)]
    names = [nm for nm, _ in _weights(family, c)]
    if family == "stem":
        nm = {"w0": "w0", "w2": [n_ for n_ in names if n_.startswith("w")][-1], "b": "b0"}[plant]
    else:
        # w2: the last block's; the QT tail's: q4's (block 1) - behind a NaN in q5's or q6's w2 the NaN gradient lies on a map's border
        # only in some channels, and torch's float32 and float64 weight gradients disagree there (G_AT)
        nm = {"w0": "w0_0", "w2": "w2_1" if family == "qtail" else [n_ for n_ in names if n_.startswith("w2")][-1], "wsc": ([n_ for n_ in names if n_.startswith("wsc")] + [None])[0]}[plant]
    a = dict(_weights(family, c))[nm]
    # the tap that reads the output's own pixel and never the zero padding: there torch's own CPU kernels disagree (one multiplies the
    # padding's zeros by the NaN, one skips them), and the float32 and float64 footprints would differ along the border
    centre = a.ndim == 4 and family != "stem"
    return [(nm, (0, 0, a.shape[2] // 2, a.shape[3] // 2) if centre else (0,) * a.ndim, NAN)]


def make(name):
    """-> the case with its plants, a dict as the family's case module makes it, plus family."""
    c = clean(name)
    arrays = dict(_weights(c["family"], c))
    for nm, idx, v in plants(name):
        (arrays[nm] if nm in arrays else c[nm])[idx] = v
    return c


def is_data_plant(name):
    return CASES[name][2] in DATA_PLANTS or CASES[name][2] == "g"


def reference_dtype(name):
    """The dtype the footprint R of a case is taken in."""
    return torch.float32 if CASES[name][2] == "overflow" else torch.float64


# ---- the ops of the two modes
class Real:
    conv = staticmethod(lambda x, w, pad, b=None: F.conv2d(x, w, b, padding=pad))
    relu = staticmethod(F.relu)
    pool = staticmethod(F.max_pool2d)
    up = staticmethod(lambda x, s: F.interpolate(x, scale_factor=s))
    add = staticmethod(lambda a, b: a + b)
    cat = staticmethod(lambda parts: torch.cat(parts, 1))
    pad = staticmethod(F.pad)


class Ind:
    """A tensor of the indicator run: f the forward indicator, g the gradient's (filled by Indicator.backward)."""

    def __init__(self, f):
        self.f, self.g = (f > 0).to(torch.float64), torch.zeros(f.shape, dtype=torch.float64)


class Indicator:
    """The ops on Ind tensors; every op notes how a gradient's indicator goes back through it."""

    def __init__(self):
        self.tape = []

    def _out(self, f, back):
        o = Ind(f)
        self.tape.append(lambda: back(o))
        return o

    def conv(self, x, w, pad, b=None):
        ones = torch.ones(w.shape, dtype=torch.float64)

        def back(o):
            x.g += F.conv_transpose2d(o.g, ones, padding=pad)
        return self._out(F.conv2d(x.f, ones, padding=pad), back)

    def relu(self, x):                  # forward: removed.  backward: the gradient is masked by the output
        def back(o):
            x.g += o.g + o.f
        return self._out(x.f, back)

    def pool(self, x, s):               # backward: routed inside the window, by the window's values
        def back(o):
            x.g += F.interpolate(o.g + o.f, scale_factor=s)
        return self._out(F.max_pool2d(x.f, s), back)

    def up(self, x, s):
        def back(o):
            x.g += F.max_pool2d(o.g, s)
        return self._out(F.interpolate(x.f, scale_factor=s), back)

    def add(self, a, b):
        def back(o):
            a.g += o.g
            b.g += o.g
        return self._out(a.f + b.f, back)

    def cat(self, parts):
        def back(o):
            lo = 0
            for p in parts:
                p.g += o.g[:, lo:lo + p.f.shape[1]]
                lo += p.f.shape[1]
        return self._out(torch.cat([p.f for p in parts], 1), back)

    def pad(self, x, pd):
        def back(o):
            hh, ww = o.g.shape[2], o.g.shape[3]
            x.g += o.g[:, :, pd[2]:hh - pd[3], pd[0]:ww - pd[1]]
        return self._out(F.pad(x.f, pd), back)

    def backward(self):
        for step in reversed(self.tape):
            step()


# ---- the nets, once
def block_net(o, x, w0, w2, wsc):
    p = w0.shape[2] // 2
    t = o.relu(o.conv(x, w0, p))
    sc = x if wsc is None else o.conv(x, wsc.reshape(wsc.shape[0], wsc.shape[1], 1, 1), 0)
    return t, o.relu(o.add(o.conv(t, w2, p), sc))


def trunk_net(o, c, x, ws, bs=None):
    """-> (named tensors a forward call writes or saves, the output the upstream gradient belongs to)"""
    r = {}
    for i, blk in enumerate(ws):
        r["t%d" % i], r["out%d" % i] = block_net(o, x, *blk)
        x = r["out%d" % i]
    r["y"] = o.pool(x, 2) if c["shape"][5] else x
    return r, r["y"]


def qtail_net(o, c, x4, ws, bs=None):
    t3, x5 = block_net(o, x4, *ws[0])
    x6 = o.cat([x5] + [o.up(o.pool(x5, s), s) for s in Q.SCALES])
    t4, x7 = block_net(o, x6, *ws[1])
    t5, o5 = block_net(o, x7, *ws[2])
    t6, x9 = block_net(o, o.pool(o5, 2), *ws[3])
    r = {"s%d" % i: a for i, a in enumerate((x4, t3, x5, t4, x7, t5, o5, t6, x9))}
    r["x9"] = x9
    return r, x9


def stem_net(o, c, x, ws, bs):
    if isinstance(o, Indicator) and c["shape"][5]:                  # the unified kernel: every tap connected
        n, h, w, cin, k, split = c["shape"]
        y = o.relu(o.conv(o.pad(x, (0, k // 2, 0, k // 2)), torch.ones(32, cin, k, k), 0))
        return {"y": y}, y
    y = o.cat([o.relu(o.conv(o.pad(x, pd), w, 0, b)) for w, b, pd in zip(ws, bs, S.pads(c["shape"]))])
    return {"y": y}, y


NET = {"block": trunk_net, "trunk": trunk_net, "qtail": qtail_net, "stem": stem_net}
G_X = {"block": "g_x", "trunk": "g_x", "qtail": "g_x4", "stem": "g_x"}


def _grad_names(family, c):
    """the flat names of the weight and bias gradients, in the order of _weights()"""
    return ["g_" + nm for nm, _ in _weights(family, c)]


def _leaves(family, c, wrap):
    if family == "stem":
        return [wrap(a) for a in c["w"]], [wrap(a) for a in c["b"]]
    return [tuple(None if a is None else wrap(a) for a in blk) for blk in c["blocks"]], None


def reference(c, dtype=torch.float64):
    """The call on the CPU as torch ops under autograd in `dtype` -> name -> numpy array, every tensor the forward and the backward call
    write: the family's flat() names (trunk_cases.flat, qtail_cases.flat, stem_cases.flat; a block is a trunk: t0, out0, y = out0)."""
    family = c["family"]
    wrap = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dtype).requires_grad_()
    x = wrap(c[X_OF[family]])
    ws, bs = _leaves(family, c, wrap)
    r, y = NET[family](Real, c, x, ws, bs)
    leaves = [x] + ([a for a in ws] + bs if family == "stem" else [a for blk in ws for a in blk if a is not None])
    grads = torch.autograd.grad([y], leaves, [torch.from_numpy(np.ascontiguousarray(c[G_OF[family]])).to(dtype)])
    out = {k: v.detach().numpy() for k, v in r.items()}
    out.update(zip([G_X[family]] + _grad_names(family, c), [g.numpy() for g in grads]))
    return out


def footprints(result):
    """name -> bool array: where a result (the reference's or a call's) is not finite."""
    return {k: ~np.isfinite(v) for k, v in result.items()}


def reach(name):
    """S of a case -> name -> bool array, reference()'s names."""
    family = CASES[name][0]
    c = clean(name)
    planted = {}
    for nm, idx, _ in plants(name):
        planted.setdefault(nm, []).append(idx)

    def indicator(a, nm):
        f = torch.zeros(a.shape, dtype=torch.float64)
        for idx in planted.get(nm, []):
            f[idx] = 1
        return f

    o = Indicator()
    x = Ind(indicator(c[X_OF[family]], X_OF[family]))
    keep = lambda a: torch.from_numpy(a)                             # weights: their shapes only
    ws, bs = _leaves(family, c, keep)
    r, y = NET[family](o, c, x, ws, bs)
    y.g += indicator(c[G_OF[family]], G_OF[family])
    o.backward()
    whole = any(nm not in (X_OF[family], G_OF[family]) for nm in planted)
    out = {k: (v.f > 0).numpy() | whole for k, v in r.items()}
    out[G_X[family]] = (x.g > 0).numpy() | whole
    for nm, (_, a) in zip(_grad_names(family, c), _weights(family, c)):
        out[nm] = np.ones(a.shape, bool)
    return out


# ---- the heads and the gate (include/pmp.h: pmp_head_*, pmp_gate_*).  Linear calls - a 3x3 convolution with a bias, the carry into channel
# 0, the attention input cat[up(q), up(y)], and an elementwise product - so a table, a reference and a reach of their own, on the same
# two modes of ops.  A head has two upstream gradients (g_y, g_att) and three data inputs (x, prev, q).
import head_cases as H  # noqa: E402

# name -> head_cases' spec (shape, prev, want_g_x, want_g_q): f_b1 and f_b2 of head_cases, and conv_q2's one 8x8 map
HEAD_SHAPES = {"f_b1": H.FLOAT_SHAPES["f_b1"], "f_b2": H.FLOAT_SHAPES["f_b2"], "q2": ((1, 8, 8, 8, 1, 0, 0), False, True, False)}
HEAD_X_PLANTS = ("nan_corner", "nan_seam", "pinf", "ninf", "pair")


def head_plants_of(nm):
    shape, prev = HEAD_SHAPES[nm][:2]
    return list(HEAD_X_PLANTS) + (["prev"] if prev else []) + (["q", "g_att"] if shape[6] else []) + ["g", "w", "b"]


HEAD_CASES = {"head-%s-%s" % (nm, p): (nm, p) for nm in HEAD_SHAPES for p in head_plants_of(nm)}


def head_clean(name):
    """head_cases.make_case of the shape, kind randn (for f_b1 and f_b2: head_cases.FLOAT's f_b1_randn and f_b2_randn themselves)"""
    nm = HEAD_CASES[name][0]
    return H.make_case(nm, "randn", spec=HEAD_SHAPES[nm])


def head_plants(name):
    nm, plant = HEAD_CASES[name]
    n, h, w, cin, cout, up_q, up_y = HEAD_SHAPES[nm][0]
    iy, ix = h // 2 + 1, w // 2 - 3
    if plant == "nan_corner":
        return [("x", (0, 0, 0, 0), NAN)]
    if plant == "nan_seam":
        return [("x", (0, 1, min(15, h - 1), min(15, w - 1)), NAN)]
    if plant in ("pinf", "ninf"):
        return [("x", (0, 1, iy, ix), INF if plant == "pinf" else -INF)]
    if plant == "pair":
        return [("x", (0, 1, iy, ix), INF), ("x", (0, 1, iy, ix + 1), -INF)]
    return {"prev": [("prev", (0, 0, iy, ix), NAN)], "q": [("q", (0, 0, 1, 2), NAN)], "g": [("g_y", (0, 0, 3, 4), NAN)],
            "g_att": [("g_att", (0, 1, 3, 4), NAN)], "w": [("w", (0, 0, 1, 1), NAN)], "b": [("b", (0,), NAN)]}[plant]


def head_make(name):
    c = head_clean(name)
    for nm, idx, v in head_plants(name):
        c[nm][idx] = v
    return c


def _slice(x, lo, hi):
    return x[:, lo:hi]


Real.slice = staticmethod(_slice)


def _ind_slice(self, x, lo, hi):
    def back(o):
        x.g[:, lo:hi] += o.g
    return self._out(x.f[:, lo:hi], back)


Indicator.slice = _ind_slice


def head_net(o, shape, x, w, b, prev, q):
    """-> (y, att or None): Model_QBD's conv_B*, the in-place carry into channel 0, F.interpolate and torch.cat"""
    cout, up_q, up_y = shape[4], shape[5], shape[6]
    y = o.conv(x, w, 1, b)
    if prev is not None:
        y = o.cat([o.add(o.slice(y, 0, 1), o.slice(prev, 0, 1)), o.slice(y, 1, cout)])
    return y, (o.cat([o.up(q, up_q), o.up(y, up_y)]) if up_y else None)


def head_reference(c, dtype=torch.float64):
    """The head under autograd -> head_cases.OUT_KEYS (None where the shape has none); every gradient, asked for or not."""
    leaf = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dtype).requires_grad_()
    plain = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dtype)
    x, w, b, prev, q = (leaf(c[k]) for k in ("x", "w", "b", "prev", "q"))
    y, att = head_net(Real, c["shape"], x, w, b, prev, q)
    outs, gs = [y], [plain(c["g_y"])]
    if att is not None:
        outs.append(att)
        gs.append(plain(c["g_att"]))
    names = [(k, t) for k, t in (("g_x", x), ("g_w", w), ("g_b", b), ("g_prev", prev), ("g_q", q)) if t is not None]
    grads = torch.autograd.grad(outs, [t for _, t in names], gs)
    r = dict.fromkeys(H.OUT_KEYS)
    r.update(y=y.detach().numpy(), att=None if att is None else att.detach().numpy())
    r.update({k: g.numpy() for (k, _), g in zip(names, grads)})
    return r


def head_reach(name):
    c = head_clean(name)
    planted = {}
    for nm, idx, _ in head_plants(name):
        planted.setdefault(nm, []).append(idx)

    def ind(nm):
        if c[nm] is None:
            return None
        f = torch.zeros(c[nm].shape, dtype=torch.float64)
        for idx in planted.get(nm, []):
            f[idx] = 1
        return Ind(f)

    o = Indicator()
    x, prev, q = ind("x"), ind("prev"), ind("q")
    y, att = head_net(o, c["shape"], x, torch.from_numpy(c["w"]), None, prev, q)
    y.g += ind("g_y").f
    if att is not None:
        att.g += ind("g_att").f
    o.backward()
    whole = "w" in planted or "b" in planted
    r = dict.fromkeys(H.OUT_KEYS)
    r.update(y=(y.f > 0).numpy() | whole, att=None if att is None else (att.f > 0).numpy() | whole, g_x=(x.g > 0).numpy() | whole,
             g_w=np.ones(c["w"].shape, bool), g_b=np.ones(c["b"].shape, bool))
    if prev is not None:
        r["g_prev"] = (prev.g > 0).numpy() | whole
    if q is not None:
        r["g_q"] = (q.g > 0).numpy() | whole
    return r


# the gate: y = x * a, g_a = g_y * x, g_x = [g_acc +] g_y * a, elementwise.  count -> the planted element: a one-element call, the last
# element of a 255-element call and of one that ends one element into its fifth block of 256
GATE_COUNTS = {1: 0, 255: 254, 1025: 1024}
GATE_PLANTS = [(k, v) for k in ("x", "a", "g_y", "g_acc") for v in (NAN, INF)]


def gate_make(count, key, value):
    """-> (head_cases.gate_case with the plant, the outputs that read the planted tensor)"""
    c = H.gate_case(count)
    c[key][GATE_COUNTS[count]] = value
    return c, {"x": ("y", "g_a"), "a": ("y", "g_x"), "g_y": ("g_a", "g_x"), "g_acc": ("g_x",)}[key]
