"""An MTT net's heads for training (include/pmp.h: pmp_head_*, pmp_gate_*): cases and float64 machinery only, shared by
tests/test_head_cases_cpu.py, tests/test_gpu_head_grad.py and tools/gen_golden_head.py.

A case is shape = (n, h, w, cin, cout, up_q, up_y) with the flags prev (the carry), want_g_x and want_g_q.  forward() and backward()
restate every formula of the header in numpy float64, written out tap by tap and window by window, no autograd:
    y   = conv3x3(x, w, pad 1) + b;  y[:, 0] += prev[:, 0];  att = cat[nearest(q, up_q), nearest(y, up_y)]
    gy  = g_y + the up_y x up_y window sums of g_att[:, 1:]            g_prev[:, 0] = gy[:, 0], zero elsewhere
    g_x = conv3x3 of gy with the mirrored, transposed w                g_w, g_b = the sums over pixels of gy * x and of gy
    g_q = the up_q x up_q window sums of g_att[:, 0]
The golden file g19_head_grad.npz holds the same quantities from the reference's own statements (nn.Conv2d, the in-place carry,
F.interpolate, torch.cat) under autograd (tools/gen_golden_head.py).

EXACT cases: x integers 0..15, w in {-1, 0, 1}, b, prev, q, g_y and g_att integers in -3..3; worst_partial_sum() stays below 2^24, so
float32 arithmetic in ANY order equals float64 bit for bit.  Shapes: one 8x8 map at n = 1; 16x24 and 24x16 (two 16-tiles one way, three
8-tiles the other, h != w); n = 3; a side of 256 as (1, 256, 8); cin 1, 5, 8, 16; cout 1 and 2; with and without prev; up (0,0), (2,1),
(4,2); g_x and g_q asked for and not; 1, 2, 255, 256 and 258 items of the weight gradient's reduction (csrc/head_train.hip: the items
are 8x8 tiles, NP = min(ceil(items / 2), 128) - just below, at and above twice the cap; 257 is prime and above n's limit).
ORDER cases (float): w is zero but for the centre tap of channel 0, which is 1, so acc = x exactly and y = (x + b) + prev is two float32
additions that numpy repeats bit for bit - the carry BEHIND the bias - on values where the other order rounds differently.
FLOAT cases, on two shapes: randn (normal), positive (log-uniform 2^-6..2^6, one sign), wide (magnitudes 2^-20..2^8, random signs, one
value in eight zero).  Weights normal / sqrt(9 cin).

BOUND of the float cases, per element, oracle/layers64.py's form:
    |gpu - ref64| <= c * 2^-24 * A + 2^-23 * |ref64|
A: the same operation on the absolute values of its inputs.  emulate() follows the header's orders of summation in float32 (a fused
multiply-add as float32(float64(acc) + the exact product)); its largest error on this table, in units of 2^-24 * A:
    C_Y_EMULATED   = 8.6   (8.52: f_b1_wide, 72 terms of 28 binades and both signs; 7.72 on f_b2_wide, 2.6-4.4 on the others)
    C_GX_EMULATED  = 4.6   (4.54: f_b1_wide; 1.6-3.3 on the others)
    C_GW_EMULATED  = 3.9   (3.85: f_b1_positive, 64 pixels of one sign per item; 3.77 on f_b2_positive, 0.2-3.2 on the others)
    C_GB_EMULATED  = 2.7   (2.61: f_b1_positive; 0.03-1.9 on the others)
c = 2 * the emulated figure; tests/test_head_cases_cpu.py asserts that the emulation stays within half of each bound.  att is y's and
q's bits; g_prev and g_q are chains of float32 additions without a product, which numpy repeats: they are held to the emulation bit
for bit (that is what pins the ORDER of the windows).
Largest |gpu - ref64| / bound on an MI355X (tests/test_gpu_head_grad.py prints them under `pytest -s`):
    y 0.453 (f_b1_wide)   g_x 0.423 (f_b1_wide)   g_w 0.392 (f_b1_positive)   g_b 0.353 (f_b1_positive)
On every float case the GPU's y, g_x, g_w and g_b equal the emulation bit for bit: it stays below half of each bound as the emulation does.
"""
import functools
import os

import numpy as np

from cases_common import as_f32, ratio, same_bits  # noqa: F401

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g19_head_grad.npz")
EPS = 2.0 ** -24
R_STORE = 2.0 ** -23
C_Y_EMULATED, C_GX_EMULATED, C_GW_EMULATED, C_GB_EMULATED = 8.6, 4.6, 3.9, 2.7
C_OF = {"y": 2 * C_Y_EMULATED, "g_x": 2 * C_GX_EMULATED, "g_w": 2 * C_GW_EMULATED, "g_b": 2 * C_GB_EMULATED}
NP_CAP = 128

# name -> (shape, prev, want_g_x, want_g_q)
EXACT = {
    "one_8x8":     ((1, 8, 8, 8, 2, 0, 0), False, True, False),         # 1 item
    "q2_8x8":      ((1, 8, 8, 8, 1, 0, 0), False, True, False),         # conv_q2's shape
    "two_items":   ((1, 8, 16, 1, 2, 2, 1), False, False, True),        # 2 items
    "b1_16x24":    ((2, 16, 24, 8, 2, 2, 1), False, True, True),        # conv_B1: attention input at the head's own resolution
    "b2_24x16":    ((3, 24, 16, 8, 2, 4, 2), True, True, True),         # conv_B2: carry and a twofold attention input
    "b2_no_gq":    ((1, 16, 16, 5, 2, 4, 2), True, True, False),
    "b3_16x16":    ((3, 16, 16, 8, 2, 0, 0), True, False, False),       # conv_B3: carry only
    "c16_att1":    ((2, 16, 8, 16, 1, 2, 1), True, True, True),         # the widest input, one output, three channels of att
    "side_256":    ((1, 256, 8, 5, 2, 4, 2), False, True, True),
    "cap_255":     ((255, 8, 8, 1, 2, 0, 0), True, True, False),        # NP = 128, the last partition adds one item
    "cap_256":     ((32, 16, 32, 2, 1, 2, 1), False, False, True),      # NP = 128, two items each
    # 257 items do not exist (257 is prime and n ends at 256): 258 = 43 * 6 is the first count above twice the cap
    "cap_258":     ((43, 8, 48, 1, 2, 4, 2), True, True, True),         # NP = 128, partitions 0 and 1 add three items
}
IN_GOLDEN = ("one_8x8", "b1_16x24", "b2_no_gq", "b3_16x16")
ORDER = {"carry_b2": ((2, 16, 16, 1, 2, 4, 2), True, True, True), "carry_b3": ((1, 8, 24, 1, 1, 0, 0), True, False, False)}
FLOAT_SHAPES = {"f_b1": ((2, 16, 24, 8, 2, 2, 1), False, True, True), "f_b2": ((3, 24, 16, 8, 2, 4, 2), True, True, True)}
KINDS = ("randn", "positive", "wide")
FLOAT = {"%s_%s" % (nm, kind): (nm, kind) for nm in FLOAT_SHAPES for kind in KINDS}
OUT_KEYS = ("y", "att", "g_x", "g_w", "g_b", "g_q", "g_prev")


def _seed(name):
    return 50021 + sum((i + 1) * ord(ch) for i, ch in enumerate(name))


def sizes(shape):
    """name -> the shape of every tensor of a head call (att, q: None without an attention input)."""
    n, h, w, cin, cout, up_q, up_y = shape
    att = (n, 1 + cout, up_y * h, up_y * w) if up_y else None
    q = (n, 1, up_y * h // up_q, up_y * w // up_q) if up_y else None
    return {"x": (n, cin, h, w), "w": (cout, cin, 3, 3), "b": (cout,), "prev": (n, cout, h, w), "y": (n, cout, h, w), "q": q, "att": att,
            "g_y": (n, cout, h, w), "g_att": att, "g_x": (n, cin, h, w), "g_w": (cout, cin, 3, 3), "g_b": (cout,), "g_q": q,
            "g_prev": (n, cout, h, w)}


def head_np(shape):
    """csrc/head_train.hip head_np -> (items, NP)."""
    items = shape[0] * (shape[1] // 8) * (shape[2] // 8)
    return items, min((items + 1) // 2, NP_CAP)


def make_case(name, kind="exact", spec=None):
    """-> dict(shape, prev_given, want_g_x, want_g_q, x, w, b, prev, q, g_y, g_att): float32 numpy arrays, None where absent."""
    if spec is None:
        spec = EXACT[name] if name in EXACT else ORDER[name] if name in ORDER else FLOAT_SHAPES[name]
    shape, has_prev, want_g_x, want_g_q = spec
    rng = np.random.default_rng(_seed(name + "/" + kind))
    sz = sizes(shape)
    ri = lambda lo, hi, s: rng.integers(lo, hi + 1, s).astype(np.float32)
    rn = lambda scale, s: (rng.standard_normal(s) * scale).astype(np.float32)
    logu = lambda lo, hi, s: (2.0 ** rng.uniform(lo, hi, s)).astype(np.float32)

    def wide(s):
        v = logu(-20, 8, s) * np.where(rng.integers(0, 2, s) == 0, -1, 1).astype(np.float32)
        return np.where(rng.integers(0, 8, s) == 0, np.float32(0), v)

    data = ("x", "prev", "q", "g_y", "g_att")
    if kind == "exact":
        c = {k: ri(-3, 3, sz[k]) for k in data if sz[k]}
        c.update(x=ri(0, 15, sz["x"]), w=ri(-1, 1, sz["w"]), b=ri(-3, 3, sz["b"]))
    elif kind == "order":
        c = {k: rn(1.0, sz[k]) for k in data if sz[k]}
        c["x"], c["prev"] = rn(1.0, sz["x"]), logu(-3, 12, sz["prev"])
        c["w"] = np.zeros(sz["w"], np.float32)
        c["w"][:, 0, 1, 1] = 1
        c["b"] = np.array([2.0 ** 12 + 0.37, -1.0 / 3][:shape[4]], np.float32)
    else:
        gen = {"randn": lambda s: rn(1.0, s), "positive": lambda s: logu(-6, 6, s), "wide": wide}[kind]
        c = {k: gen(sz[k]) for k in data if sz[k]}
        c.update(w=rn((9 * shape[3]) ** -0.5, sz["w"]), b=rn(1.0, sz["b"]))
    for k in ("q", "g_att"):
        c.setdefault(k, None)
    if not has_prev:
        c["prev"] = None
    c.update(shape=shape, want_g_x=want_g_x, want_g_q=want_g_q)
    return c


# ---- the float64 restatement
def _f(a, absolute):
    a = np.asarray(a, np.float64)
    return np.abs(a) if absolute else a


def windows(a, u):
    """[..., u H, u W] -> the list of its u x u window planes [..., H, W] in row-major order."""
    return [a[..., i::u, j::u] for i in range(u) for j in range(u)]


def up(a, u):
    return a.repeat(u, axis=-2).repeat(u, axis=-1)


def forward(c, absolute=False):
    """-> dict(y, att) in float64.  absolute: the companion on magnitudes (the A of the bound)."""
    n, h, w, cin, cout, up_q, up_y = c["shape"]
    x, wt, b = _f(c["x"], absolute), _f(c["w"], absolute), _f(c["b"], absolute)
    xp = np.pad(x, ((0, 0), (0, 0), (1, 1), (1, 1)))
    y = np.zeros((n, cout, h, w))
    for ci in range(cin):
        for dy in range(3):
            for dx in range(3):
                y += wt[None, :, ci, dy, dx, None, None] * xp[:, ci, None, dy:dy + h, dx:dx + w]
    y = y + b[None, :, None, None]
    if c["prev"] is not None:
        y[:, 0] = y[:, 0] + _f(c["prev"], absolute)[:, 0]
    att = np.concatenate([up(_f(c["q"], absolute), up_q), up(y, up_y)], 1) if up_y else None
    return {"y": y, "att": att}


def effective(c, absolute=False):
    """gy: g_y and, behind it, the window of g_att in the order (0,0), (0,1), (1,0), (1,1)."""
    gy = _f(c["g_y"], absolute).copy()
    if c["shape"][6]:
        for win in windows(_f(c["g_att"], absolute)[:, 1:], c["shape"][6]):
            gy = gy + win
    return gy


def backward(c, absolute=False):
    """-> dict(g_x, g_w, g_b, g_q, g_prev) in float64, every one of them whether the case asks for it or not (g_q: None without an
    attention input)."""
    n, h, w, cin, cout, up_q, up_y = c["shape"]
    x, wt = _f(c["x"], absolute), _f(c["w"], absolute)
    gy = effective(c, absolute)
    xp, gp = np.pad(x, ((0, 0), (0, 0), (1, 1), (1, 1))), np.pad(gy, ((0, 0), (0, 0), (1, 1), (1, 1)))
    g_x, g_w = np.zeros((n, cin, h, w)), np.zeros((cout, cin, 3, 3))
    for co in range(cout):
        for dy in range(3):
            for dx in range(3):
                g_x += wt[None, co, :, dy, dx, None, None] * gp[:, co, None, 2 - dy:2 - dy + h, 2 - dx:2 - dx + w]
                g_w[co, :, dy, dx] = (gy[:, co, None] * xp[:, :, dy:dy + h, dx:dx + w]).sum((0, 2, 3))
    g_prev = np.zeros_like(gy)
    g_prev[:, 0] = gy[:, 0]
    g_q = sum(windows(_f(c["g_att"], absolute)[:, :1], up_q)) if up_y else None
    return {"g_x": g_x, "g_w": g_w, "g_b": gy.sum((0, 2, 3)), "g_q": g_q, "g_prev": g_prev}


def restate(c, absolute=False):
    return dict(forward(c, absolute), **backward(c, absolute))


def asked(c, r):
    """r without what the case does not ask for: g_x, g_q, and g_prev without a carry."""
    r = dict(r)
    if not c["want_g_x"]:
        r["g_x"] = None
    if not c["want_g_q"]:
        r["g_q"] = None
    if c["prev"] is None:
        r["g_prev"] = None
    return r


def worst_partial_sum(c):
    """The largest sum of |term| over the elements of every operation of a case: a bound on every partial sum, whatever the order."""
    return max(float(v.max()) for v in restate(c, absolute=True).values() if v is not None)


@functools.lru_cache(maxsize=None)
def exact(name):
    """-> (case, the float64 restatement as the float32 a kernel must produce, None for what is not asked for); computed once."""
    c = make_case(name)
    return c, {k: as_f32(v) for k, v in asked(c, restate(c)).items()}


# ---- the header's orders of summation in float32 on the CPU
def _fma(acc, a, b):
    """float32 acc + a * b with one rounding (up to a double rounding): the product of two float32 is exact in float64."""
    return (acc.astype(np.float64) + np.asarray(a, np.float64) * np.asarray(b, np.float64)).astype(np.float32)


def emulate_effective(c):
    gy = np.asarray(c["g_y"], np.float32).copy()
    if c["shape"][6]:
        for win in windows(np.asarray(c["g_att"], np.float32)[:, 1:], c["shape"][6]):
            gy = gy + win                                             # float32 + float32: one rounding each, in the header's order
    return gy


def emulate(c):
    """-> dict like restate(), float32, following include/pmp.h's orders."""
    n, h, w, cin, cout, up_q, up_y = c["shape"]
    x, wt = np.asarray(c["x"], np.float32), np.asarray(c["w"], np.float32)
    xp = np.pad(x, ((0, 0), (0, 0), (1, 1), (1, 1)))
    acc = np.zeros((n, cout, h, w), np.float32)
    for ci in range(cin):
        for dy in range(3):
            for dx in range(3):
                acc = _fma(acc, wt[None, :, ci, dy, dx, None, None], xp[:, ci, None, dy:dy + h, dx:dx + w])
    y = acc + np.asarray(c["b"], np.float32)[None, :, None, None]
    if c["prev"] is not None:
        y[:, 0] = y[:, 0] + np.asarray(c["prev"], np.float32)[:, 0]
    att = np.concatenate([up(np.asarray(c["q"], np.float32), up_q), up(y, up_y)], 1) if up_y else None
    gy = emulate_effective(c)
    gp = np.pad(gy, ((0, 0), (0, 0), (1, 1), (1, 1)))
    g_x = np.zeros((n, cin, h, w), np.float32)
    for co in range(cout):
        for dy in range(3):
            for dx in range(3):
                g_x = _fma(g_x, wt[None, co, :, dy, dx, None, None], gp[:, co, None, 2 - dy:2 - dy + h, 2 - dx:2 - dx + w])
    # stage 1: partition p adds the items p, p + NP, ... pixel by pixel in row order; stage 2: the partials in the order 0 .. NP-1
    items, NP = head_np(c["shape"])
    tiles_x, tiles = w // 8, (w // 8) * (h // 8)
    acc_w, acc_b = np.zeros((NP, cout, cin, 3, 3), np.float32), np.zeros((NP, cout), np.float32)
    for first in range(0, items, NP):
        xt, gt = np.zeros((NP, cin, 10, 10), np.float32), np.zeros((NP, cout, 8, 8), np.float32)
        for p, it in enumerate(range(first, min(first + NP, items))):    # a partition without an item in this round adds +0 products
            nn, tt = divmod(it, tiles)
            ty, tx = divmod(tt, tiles_x)
            xt[p], gt[p] = xp[nn, :, ty * 8:ty * 8 + 10, tx * 8:tx * 8 + 10], gy[nn, :, ty * 8:ty * 8 + 8, tx * 8:tx * 8 + 8]
        for yy in range(8):
            for xx in range(8):
                gv = gt[:, :, yy, xx]
                acc_w = _fma(acc_w, gv[:, :, None, None, None], xt[:, None, :, yy:yy + 3, xx:xx + 3])
                acc_b = acc_b + gv
    g_w, g_b = acc_w[0], acc_b[0]
    for p in range(1, NP):
        g_w, g_b = g_w + acc_w[p], g_b + acc_b[p]
    g_q = None
    if up_y:
        g_q = np.zeros(sizes(c["shape"])["q"], np.float32)
        for win in windows(np.asarray(c["g_att"], np.float32)[:, :1], up_q):
            g_q = g_q + win
    g_prev = np.zeros_like(gy)
    g_prev[:, 0] = gy[:, 0]
    return {"y": y, "att": att, "g_x": g_x, "g_w": g_w, "g_b": g_b, "g_q": g_q, "g_prev": g_prev}


BOUNDED = ("y", "g_x", "g_w", "g_b")          # held to the bound; att, g_q and g_prev bit for bit to the emulation


@functools.lru_cache(maxsize=None)
def float_reference(name):
    """-> (case, ref, bound, emulated): float64 reference and per-element bounds of BOUNDED, and the float32 emulation of everything."""
    nm, kind = FLOAT[name]
    c = make_case(nm, kind)
    ref, A = restate(c), restate(c, absolute=True)
    bound = {k: C_OF[k] * EPS * A[k] + R_STORE * np.abs(ref[k]) for k in BOUNDED}
    return c, ref, bound, A, emulate(c)


# ---- the gate: x * a, g_y * x, [g_acc +] g_y * a in numpy float32, one rounding per operation
GATE_COUNTS = (1, 3, 4, 1023, 2 ** 20 + 5)


def gate_case(count, seed=0):
    """Random finite float32 bit patterns' worth of values: normals of every magnitude that cannot overflow a product or a sum,
    subnormals, +0 and -0."""
    rng = np.random.default_rng(977 + count + seed)
    out = {}
    for k in ("x", "a", "g_y", "g_acc"):
        v = (2.0 ** rng.uniform(-60, 60, count) * np.where(rng.integers(0, 2, count) == 0, -1, 1)).astype(np.float32)
        kind = rng.integers(0, 16, count)
        v = np.where(kind == 0, np.float32(0.0), v)
        v = np.where(kind == 1, np.float32(-0.0), v)
        sub = (rng.integers(1, 2 ** 23, count).astype(np.uint32) | (rng.integers(0, 2, count).astype(np.uint32) << 31)).view(np.float32)
        out[k] = np.where(kind == 2, sub, v).astype(np.float32)
    return out


def gate_reference(c, with_acc):
    with np.errstate(under="ignore"):
        v = c["g_y"] * c["a"]
        return {"y": c["x"] * c["a"], "g_a": c["g_y"] * c["x"], "g_x": c["g_acc"] + v if with_acc else v}
