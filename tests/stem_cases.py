"""The nets' first layers for training (include/pmp.h: pmp_stem_*): cases and float64 machinery only, shared by
tests/test_stem_cases_cpu.py, tests/test_gpu_stem_grad.py and tools/gen_golden_stem.py.

A case is (n, h, w, cin, k, split).  With p = k // 2, x is [n, cin, h + p, w + p] - a net's input before its right / bottom padding -
and convs one (w, b) pair (split 0: w [32, cin, k, k]) or three (split 1: [16, cin, k, k], [8, cin, p + 1, k], [8, cin, k, p + 1]).
forward() is written as the reference writes it (Model_QBD.py:79-80, :132-135): F.pad per convolution, conv2d, cat, relu.  backward()
is written out, not taken from autograd: gm = g_y where y > 0, else 0; per convolution the weight gradient, the bias gradient as a sum
and the input gradient as a transposed convolution cropped back to x.  unified() is the other statement - ONE k x k convolution with
32 outputs whose smaller kernels are zero-padded - which csrc/stem_train.hip computes.

EXACT cases: every value an integer - pixels 0..255 in the image channels, 0..3 in the last channel of a split stem (the QT map),
+-1 weights, biases in -3..3, g_y in {-1, 0, 1} (with `sparse`, one in sixteen non-zero) - and worst_partial_sum() below 2^24, so that
float32 arithmetic in ANY order equals float64 bit for bit; about half of y is zero and exercises the `> 0` mask.
  q_luma_one   one tile, every halo pixel is padding          m_luma   odd n, non-square the other way, 5x9 against 9x5
  parts1..3    1, 2 and 3 work items of the weight gradient's reduction, cin = 4, k = 9, split: the widest accumulator set
  cap_1023, cap_1025   just below and just above 2 * 512 work items, the cap of stem_np() (csrc/stem_train.hip: NP =
               min(ceil(items / 2), 512)): 512 partial sums of two items each but the last, and 512 of which the first adds three
FLOAT cases, name -> (shape, kind), on two shapes:
  randn     normal x and g_y                 positive  x and g_y log-uniform in 2^-6 .. 2^6, one sign: the worst chain for g_w
  pixels    image channels integers 0..255 (the last channel of a split stem 0..3), normal g_y
weights normal / sqrt(fan-in), biases normal; y reaches the backward pass as the float32 rounding of the float64 forward, so gm is exact.

BOUND of the float cases, per element, in tests/grad_cases.py's form:
    |gpu - ref64| <= c * 2^-24 * A  +  2^-23 * |ref64|
A: the same operation on the absolute values of its inputs.  No P term: gm is exact and nothing else is computed on the way.
c per kernel, derived the way grad_cases derived C_WGRAD: emulate_*() follow the order of additions documented in the header of
csrc/stem_train.hip in float32 - forward: acc = b, then one fused multiply-add per reduction index r = (ci, dy, dx) in order; weight
and bias gradient: workgroup q of NP adds the items q, q + NP, ... pixel by pixel in row order, then the NP partials in the order
0 .. NP-1; input gradient: one chain over (co, dy, dx) - and on the float cases of this table their error reaches
    C_FWD_EMULATED   = 7.0   (6.97: y of f_luma_pixels; 3.8-6.2 on the others)
    C_WGRAD_EMULATED = 12.5  (12.45: g_w1 of f_luma_positive, 256 pixels of one sign per workgroup; 9.2 on f_chroma_positive,
                              1.4-1.9 on randn and pixels; the bias gradients 0.3-6.3)
    C_DGRAD_EMULATED = 7.7   (7.61: g_x of f_chroma_positive, one chain of 800 terms; 2.6-7.2 on the others)
in units of 2^-24 * A (the final rounding of the result included, which the second term of the bound covers once more).
c = 2 * the emulated figure (layers64's margin for the order inside an MFMA; on gfx950 an fp32 MFMA is documented as a k-ordered
chain of fused multiply-adds, so the GPU is expected near the emulation).  tests/test_stem_cases_cpu.py asserts that the emulation
stays within half of each bound.
Largest |gpu - ref64| / bound on an MI355X (tests/test_gpu_stem_grad.py prints them under `pytest -s`):
    stem_forward_kernel 0.46 (f_luma_pixels; 0.26-0.40 on the others)     stem_wgrad_kernel + stem_reduce_kernel 0.46
    (f_luma_positive; 0.34 on f_chroma_positive, 0.06-0.07 on randn and pixels)     stem_dgrad_kernel 0.46 (f_chroma_positive; 0.44
    on f_luma_positive, 0.16-0.22 on the others): the GPU stays below half of each bound, as the emulation does by construction.

THE SWEEP over every shape the header accepts - all sixteen (cin, k, split), sides and n of 256, the cap of the partition with the wide
accumulator sets, masks on the edge of `> 0`, subnormals, float cases with a real second-stage chain - is tests/stem_sweep_cases.py,
built on this module's machinery, with constants of its own; the cases and constants here stay as they are.
"""
import functools
import os

import numpy as np
import torch
import torch.nn.functional as F

from cases_common import as_f32, ratio, same_bits  # noqa: F401 (S.as_f32, S.ratio, S.same_bits)

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g18_stem_grad.npz")
EPS = 2.0 ** -24
R_STORE = 2.0 ** -23
C_FWD_EMULATED = 7.0
C_WGRAD_EMULATED = 12.5
C_DGRAD_EMULATED = 7.7
C_FWD, C_WGRAD, C_DGRAD = 2 * C_FWD_EMULATED, 2 * C_WGRAD_EMULATED, 2 * C_DGRAD_EMULATED
NP_CAP = 512

# name -> (n, h, w, cin, k, split)
EXACT = {
    "q_luma_one":   (1, 16, 16, 1, 9, 0),
    "q_luma_tiles": (2, 32, 48, 1, 9, 0),
    "m_luma":       (3, 48, 16, 2, 9, 1),
    "q_chroma":     (2, 16, 32, 3, 5, 0),
    "m_chroma":     (2, 32, 32, 4, 5, 1),
    "m_luma_64":    (1, 64, 64, 2, 9, 1),
    "parts1":       (1, 16, 16, 4, 9, 1),
    "parts2":       (1, 16, 32, 4, 9, 1),
    "parts3":       (1, 16, 48, 4, 9, 1),
    "cap_1023":     (31, 48, 176, 1, 5, 0),       # 31 * 3 * 11 items: NP = 512, the last workgroup adds one item
    "cap_1025":     (41, 80, 80, 1, 5, 0),        # 41 * 25 items: NP = 512, workgroup 0 adds three
}
SPARSE = ("cap_1023", "cap_1025")                 # g_y non-zero on one pixel in sixteen: 255 * pixels / 16 stays below 2^24
IN_GOLDEN = ("q_luma_one", "m_luma", "q_chroma")
FLOAT_SHAPES = {"f_luma": (2, 32, 16, 2, 9, 1), "f_chroma": (3, 16, 32, 3, 5, 0)}
KINDS = ("randn", "positive", "pixels")
FLOAT = {"%s_%s" % (nm, kind): (nm, kind) for nm in FLOAT_SHAPES for kind in KINDS}


def _seed(name):
    return 20239 + sum((i + 1) * ord(ch) for i, ch in enumerate(name))


def conv_shapes(shape):
    """-> [(cout, cin, kh, kw)] of the stem's one or three convolutions."""
    n, h, w, cin, k, split = shape
    p = k // 2
    return [(16, cin, k, k), (8, cin, p + 1, k), (8, cin, k, p + 1)] if split else [(32, cin, k, k)]


def pads(shape):
    """F.pad's (left, right, top, bottom) of each convolution: padding_rb, padding_r, padding_b (Model_QBD.py:64-66)."""
    p = shape[4] // 2
    return [(0, p, 0, p), (0, p, 0, 0), (0, 0, 0, p)][:3 if shape[5] else 1]


def stem_np(shape):
    """csrc/stem_train.hip stem_np -> (items, NP): the work items of the weight gradient and the number of partial sums."""
    items = shape[0] * (shape[1] // 16) * (shape[2] // 16)
    return items, min((items + 1) // 2, NP_CAP)


def make_case(name, kind="exact", shape=None, sparse=None):
    """-> dict(shape, x, w [list], b [list], g_y) of float32 numpy arrays.  shape, sparse: of a case that is not in this module's
    tables (tests/stem_sweep_cases.py); the name still seeds the values."""
    if shape is None:
        shape = EXACT[name] if name in EXACT else FLOAT_SHAPES[name]
    if sparse is None:
        sparse = name in SPARSE
    n, h, w, cin, k, split = shape
    p = k // 2
    g = torch.Generator().manual_seed(_seed(name + "/" + kind))
    ri = lambda lo, hi, *s: torch.randint(lo, hi + 1, s, generator=g).to(torch.float32).numpy()
    rn = lambda scale, *s: (torch.randn(s, generator=g, dtype=torch.float64) * scale).to(torch.float32).numpy()
    logu = lambda lo, hi, *s: (2.0 ** (lo + (hi - lo) * torch.rand(s, generator=g, dtype=torch.float64))).to(torch.float32).numpy()
    sx, sy = (n, cin, h + p, w + p), (n, 32, h, w)

    def pixels():
        x = ri(0, 255, *sx)
        if split:
            x[:, -1] = ri(0, 3, n, h + p, w + p)
        return x

    shapes = conv_shapes(shape)
    if kind == "exact":
        c = {"x": pixels(), "w": [2 * ri(0, 1, *s) - 1 for s in shapes], "b": [ri(-3, 3, s[0]) for s in shapes], "g_y": ri(-1, 1, *sy)}
        if sparse:
            c["g_y"] = np.where(ri(0, 15, *sy) == 0, c["g_y"], np.float32(0))
    else:
        c = {"w": [rn((s[1] * s[2] * s[3]) ** -0.5, *s) for s in shapes], "b": [rn(1.0, s[0]) for s in shapes]}
        if kind == "randn":
            c["x"], c["g_y"] = rn(1.0, *sx), rn(1.0, *sy)
        elif kind == "positive":
            c["x"], c["g_y"] = logu(-6, 6, *sx), logu(-6, 6, *sy)
        elif kind == "pixels":
            c["x"], c["g_y"] = pixels(), rn(1.0, *sy)
        else:
            raise KeyError(kind)
    c["shape"] = shape
    return c


def _t(a, dtype=torch.float64):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype)


# ---- the restatement
def forward(c, dtype=torch.float64, absolute=False):
    """y as the reference writes it.  absolute: the companion on magnitudes, without the relu (the A of the bound)."""
    f = (lambda a: _t(np.abs(a), dtype)) if absolute else (lambda a: _t(a, dtype))
    x = f(c["x"])
    outs = [F.conv2d(F.pad(x, pd), f(w), f(b)) for w, b, pd in zip(c["w"], c["b"], pads(c["shape"]))]
    y = torch.cat(outs, 1)
    return (y if absolute else F.relu(y)).numpy()


def backward(c, y, dtype=torch.float64, absolute=False):
    """-> dict(g_x, g_w [list], g_b [list]) from the GIVEN y: written out, no autograd.  absolute: the companion on magnitudes."""
    f = (lambda a: _t(np.abs(a), dtype)) if absolute else (lambda a: _t(a, dtype))
    n, h, w, cin, k, split = c["shape"]
    p = k // 2
    x = f(c["x"])
    gm = torch.where(_t(y, dtype) > 0, f(c["g_y"]), torch.zeros((), dtype=dtype))
    r = {"g_x": torch.zeros_like(x), "g_w": [], "g_b": []}
    lo = 0
    for wt, pd in zip(c["w"], pads(c["shape"])):
        wt = f(wt)
        gj = gm[:, lo:lo + wt.shape[0]]
        lo += wt.shape[0]
        r["g_w"].append(torch.nn.grad.conv2d_weight(F.pad(x, pd), wt.shape, gj).numpy())
        r["g_b"].append(gj.sum((0, 2, 3)).numpy())
        r["g_x"] += F.conv_transpose2d(gj, wt)[:, :, :h + p, :w + p]          # the gradient of the padding is dropped
    r["g_x"] = r["g_x"].numpy()
    return r


def restate(c, dtype=torch.float64):
    y = forward(c, dtype)
    return dict(backward(c, y, dtype), y=y)


def flat(r):
    """dict(y, g_x, g_w, g_b) -> name -> array: y, g_x, g_w0.., g_b0.."""
    out = {"y": r["y"], "g_x": r["g_x"]}
    for j, (gw, gb) in enumerate(zip(r["g_w"], r["g_b"])):
        out["g_w%d" % j], out["g_b%d" % j] = gw, gb
    return out


def autograd(c):
    """The stem as float64 torch ops under autograd, the way the nets' forward writes it -> flat results (the CPU tests' yardstick
    of the restatement, here and in the sweep)."""
    d = lambda a: torch.from_numpy(np.asarray(a, np.float64).copy())
    x = d(c["x"]).requires_grad_()
    ws, bs = [d(w).requires_grad_() for w in c["w"]], [d(b).requires_grad_() for b in c["b"]]
    y = torch.cat([F.relu(F.conv2d(F.pad(x, pd), w, b)) for w, b, pd in zip(ws, bs, pads(c["shape"]))], 1)
    (y * d(c["g_y"])).sum().backward()
    num = lambda v: v.detach().numpy()
    return flat({"y": num(y), "g_x": num(x.grad), "g_w": [num(w.grad) for w in ws], "g_b": [num(b.grad) for b in bs]})


def unified(shape, ws, bs):
    """The one k x k convolution: -> (wu [32, cin, k, k], bu [32]) with the smaller kernels zero-padded (csrc/stem_train.hip)."""
    n, h, w, cin, k, split = shape
    p = k // 2
    wu = np.zeros((32, cin, k, k), np.asarray(ws[0]).dtype)
    if not split:
        wu[:] = ws[0]
    else:
        wu[:16], wu[16:24, :, :p + 1, :], wu[24:, :, :, :p + 1] = ws[0], ws[1], ws[2]
    return wu, np.concatenate([np.asarray(b) for b in bs])


def split_grads(shape, gwu, gbu):
    """The inverse on gradients: -> (g_w [list], g_b [list]); the taps outside a kernel's support are dropped."""
    p = shape[4] // 2
    if not shape[5]:
        return [gwu], [gbu]
    return [gwu[:16], gwu[16:24, :, :p + 1, :], gwu[24:, :, :, :p + 1]], [gbu[:16], gbu[16:24], gbu[24:]]


def forward_unified(c, dtype=torch.float64):
    wu, bu = unified(c["shape"], c["w"], c["b"])
    p = c["shape"][4] // 2
    return F.relu(F.conv2d(F.pad(_t(c["x"], dtype), (0, p, 0, p)), _t(wu, dtype), _t(bu, dtype))).numpy()


def worst_partial_sum(c):
    """The largest sum of |term| over the output elements of every operation of a case, each on the magnitudes of its actual inputs
    (gm behind the actual mask): a bound on every partial sum a kernel can form, whatever its order."""
    y = forward(c)
    a = backward(c, y, absolute=True)
    return max([float(forward(c, absolute=True).max()), float(a["g_x"].max())] + [float(v.max()) for v in a["g_w"] + a["g_b"]])


@functools.lru_cache(maxsize=None)
def exact(name):
    """-> (case, the float64 restatement, flat, as the float32 a kernel must produce); computed once, never changed."""
    c = make_case(name)
    return c, {k: as_f32(v) for k, v in flat(restate(c)).items()}


# ---- csrc/stem_train.hip's orders of additions in float32 on the CPU.  One rounding per term added: the product of two float32 is
# exact in float64, and acc = float32(float64(acc) + product) is the fused multiply-add up to a double rounding.
def _xp(c):
    p = c["shape"][4] // 2
    return F.pad(_t(c["x"]), (0, p, 0, p))


def emulate_forward(c):
    n, h, w, cin, k, split = c["shape"]
    wu, bu = unified(c["shape"], c["w"], c["b"])
    xp, wu = _xp(c), _t(wu)
    acc = _t(bu, torch.float32)[None, :, None, None].expand(n, 32, h, w).clone()
    for ci in range(cin):
        for dy in range(k):
            for dx in range(k):
                acc = (acc.double() + wu[None, :, ci, dy, dx, None, None] * xp[:, ci, None, dy:dy + h, dx:dx + w]).float()
    return F.relu(acc).numpy()


def emulate_wgrad(c, y):
    """-> (g_w [list], g_b [list]) in float32: stage 1 per workgroup, stage 2 over the NP partial sums in the order 0 .. NP-1."""
    n, h, w, cin, k, split = c["shape"]
    items, NP = stem_np(c["shape"])
    tiles_x, tiles = w // 16, (w // 16) * (h // 16)
    xp = _xp(c)
    gm = torch.where(_t(y) > 0, _t(c["g_y"]), torch.zeros((), dtype=torch.float64))
    acc_w = torch.zeros((NP, 32, cin, k, k), dtype=torch.float32)
    acc_b = torch.zeros((NP, 32), dtype=torch.float32)
    for first in range(0, items, NP):
        its = list(range(first, min(first + NP, items)))
        xt = torch.zeros((NP, cin, 16 + k - 1, 16 + k - 1), dtype=torch.float64)
        gt = torch.zeros((NP, 32, 16, 16), dtype=torch.float64)           # a workgroup without an item in this round adds nothing:
        for q, it in enumerate(its):                                      # +0 products leave a float32 sum as it is
            nn, tt = divmod(it, tiles)
            ty, tx = divmod(tt, tiles_x)
            xt[q] = xp[nn, :, ty * 16:ty * 16 + 16 + k - 1, tx * 16:tx * 16 + 16 + k - 1]
            gt[q] = gm[nn, :, ty * 16:ty * 16 + 16, tx * 16:tx * 16 + 16]
        for yy in range(16):
            for xx in range(16):
                gv = gt[:, :, yy, xx]
                acc_w = (acc_w.double() + gv[:, :, None, None, None] * xt[:, None, :, yy:yy + k, xx:xx + k]).float()
                acc_b = (acc_b.double() + gv).float()
    sw, sb = acc_w[0], acc_b[0]
    for q in range(1, NP):
        sw, sb = sw + acc_w[q], sb + acc_b[q]
    return split_grads(c["shape"], sw.numpy(), sb.numpy())


def emulate_dgrad(c, y):
    n, h, w, cin, k, split = c["shape"]
    p = k // 2
    wu = _t(unified(c["shape"], c["w"], c["b"])[0])
    gm = torch.where(_t(y) > 0, _t(c["g_y"]), torch.zeros((), dtype=torch.float64))
    gp = F.pad(gm, (k - 1, k - 1, k - 1, k - 1))
    acc = torch.zeros((n, cin, h + p, w + p), dtype=torch.float32)
    for co in range(32):
        for dy in range(k):
            for dx in range(k):
                gv = gp[:, co, None, k - 1 - dy:k - 1 - dy + h + p, k - 1 - dx:k - 1 - dx + w + p]
                acc = (acc.double() + wu[None, co, :, dy, dx, None, None] * gv).float()
    return acc.numpy()


# ---- float cases: the float64 reference with its per-element bounds
@functools.lru_cache(maxsize=None)
def float_reference(name):
    """-> (case, y32, ref, bound): y32 the float32 rounding of the float64 forward, which the backward pass is given; ref and bound
    float64 arrays, flat() names; the kernel of each output in KERNEL_OF."""
    nm, kind = FLOAT[name]
    c = make_case(nm, kind)
    y = forward(c)
    y32 = as_f32(y)
    ref = flat(dict(backward(c, y32), y=y))
    A = flat(dict(backward(c, y32, absolute=True), y=forward(c, absolute=True)))
    bound = {key: C_OF[KERNEL_OF(key)] * EPS * A[key] + R_STORE * np.abs(ref[key]) for key in ref}
    return c, y32, ref, bound, A


def KERNEL_OF(key):
    return "forward" if key == "y" else "dgrad" if key == "g_x" else "wgrad"


C_OF = {"forward": C_FWD, "wgrad": C_WGRAD, "dgrad": C_DGRAD}


def emulate(c, y32):
    """flat() of the three emulations."""
    g_w, g_b = emulate_wgrad(c, y32)
    return flat({"y": emulate_forward(c), "g_x": emulate_dgrad(c, y32), "g_w": g_w, "g_b": g_b})
