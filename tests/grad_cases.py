"""The sweep of the training kernels over the shapes include/pmp.h accepts: cases and float64 machinery only, shared by
tests/test_grad_cases_cpu.py, tests/test_gpu_grad_sweep.py and tools/gen_golden_grad_sweep.py.  The formulas are resblock_cases'
(forward, backward) and trunk_cases' (restate); nothing is restated a second time here.

BLOCK cases, name -> (n, h, w, cin, cout, k); the table is built by fixed cycles (no run-time draw) and every case runs.
  grid     k x pad(cin) x pad(cout), twice: `p` with the channel counts equal to the pads (equal pads: the identity shortcut), `r` with
           ragged real counts of RAGGED and cin != cout everywhere, so that the 1x1 shortcut gradient wgrad_partial_kernel<1,NCO> meets
           every (NCO, CB) too.  The maps cycle over MAPS, n over NS.
  edges    the partition of the weight gradients' reduction (conv_wgrad.hip wgrad_np: NP = min(ceil(items / 2), 256 / (Ca / 16)) partial
           sums of items = n * tiles): 1, 2 and 3 items; just below, at and just above 2 * cap for Ca = 16, 32 and 64 (257 is a prime
           above n's limit: 258 there); n = 256; a 256 x 256 map.
Every block case runs on the EXACT integers of resblock_cases (kind "exact").  FLOAT holds the cases that also run on float values,
name -> (block case, kind), every (k, NCO) pair among them, the longest chain of one workgroup 768 terms (<= 2048):
  randn     normal x and g_out
  positive  x and g_out log-uniform in 2^-6 .. 2^6, all positive: every term of g_w2 has one sign, the worst case of a float32 chain
  wide      magnitudes log-uniform in 2^-20 .. 2^8, a quarter of them zero, random signs
  border    normal, non-zero only on the two outermost rows and columns: only the halo taps of the edge tiles see anything
weights normal / sqrt(fan-in) in all four; t and out reach the backward pass as the float32 roundings of the float64 forward.
MASK_EDGES: exact cases whose t and out hold only -2^-149, -0.0, +0.0, 2^-149 and 2^-148: the masks must follow `> 0`, and g_w2 is an
integer multiple of 2^-149 below 2^-126 - an exact subnormal - while g_w0, g_wsc and g_x stay integers.

TRUNK cases, name -> (n, h, w, cin, [(cout, k), ...], pool), with trunk_cases' sparse +-1 weights (its density fits eight blocks: the largest sum
of |terms| is 7.5e6).  SUBNORMAL_TRUNK is one of them with x scaled by 2^-149: y, every t_i, out_i and weight gradient
are the unscaled case's times 2^-149 (exact subnormals: every magnitude is below 2^23), g_x and the masks are unchanged.

BOUND of the float cases, per element, in oracle/layers64.py's form:
    |gpu - ref64| <= c * 2^-24 * A  +  2^-23 * |ref64|  +  P
A: the same operation on the absolute values of its inputs; P: the bound of an input that the kernels computed themselves (t into
out; gt into g_w0 and g_x) pushed through the operation's absolute-value companion.  gu and the masks are exact.  For the
convolutions (t, out, gt, g_x) c = layers64.C_DP["fp32"] = 24: the same kernel at chains of at most 64 * 25 + 64 terms.
For the weight gradients c = C_WGRAD, derived the way layers64 derived c_dp: emulate_wgrad() follows the documented order in
float32 - workgroup p adds the items p, p + NP, ... pixel by pixel in row order, one rounding per product added (a float64 product:
the fused multiply-add), then the NP partial sums are added in the order 0 .. NP-1 - and on the float cases of this table its error
reaches
    C_WGRAD_EMULATED = 16.5 units of 2^-24 * A   (16.49: g_wsc of f_p_k5_64to32_positive, one workgroup adding 512 pixels of one
                                                  sign; 4.5-13 on the other `positive` cases, 2-10 on `wide`, 0.3-4.7 on the rest)
C_WGRAD = 2 * C_WGRAD_EMULATED = 33: the factor two is layers64's margin for the unknown order of an MFMA's four inner products.
Largest |gpu - ref64| / bound on an MI355X (tests/test_gpu_grad_sweep.py prints them under `pytest -s`), per kernel class:
    conv (t) 3x3 0.46, 5x5 0.34          conv + shortcut (out) 3x3 0.05, 5x5 0.02      data gradient (g_x) 3x3 0.10, 5x5 0.05
    wgrad_partial_kernel<1,NCO>  NCO 1: 0.27  2: 0.47  4: 0.27        <3,NCO>  0.21  0.21  0.21        <5,NCO>  0.18  0.35  0.25
(the weight gradients' largest all on `positive`, the convolutions' on `wide`): the GPU stays at or below half of each bound, as the
emulation does by construction.
"""
import functools
import os

import numpy as np
import torch
import torch.nn.functional as F

import resblock_cases as K
import trunk_cases as T
from cases_common import ratio  # noqa: F401 (G.ratio)
from oracle import layers64 as L

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g17_grad_sweep.npz")
EPS = L.EPS
C_CONV = L.C_DP["fp32"]
R_STORE = L.R_DP["fp32"]
C_WGRAD_EMULATED = 16.5
C_WGRAD = 2 * C_WGRAD_EMULATED

MAPS = ((16, 16), (32, 16), (16, 32), (48, 32), (32, 64), (16, 256), (256, 16))
NS = (1, 2, 3, 5)
PADS = (16, 32, 64)
RAGGED = {16: (1, 3, 8, 15), 32: (17, 24, 31), 64: (33, 40, 48, 49, 63)}
KINDS = ("randn", "positive", "wide", "border")
SUB = 2.0 ** -149


def pad(c):
    return 16 if c <= 16 else 32 if c <= 32 else 64


def _grid():
    cases, i, turn = {}, 0, {p: 0 for p in PADS}

    def ragged(p, other=None):
        while True:
            c = RAGGED[p][turn[p] % len(RAGGED[p])]
            turn[p] += 1
            if c != other:
                return c

    for tag in ("p", "r"):
        for k in (3, 5):
            for pci in PADS:
                for pco in PADS:
                    (h, w), n = MAPS[i % len(MAPS)], NS[i % len(NS)]
                    cin = pci if tag == "p" else ragged(pci)
                    cout = pco if tag == "p" else ragged(pco, cin)
                    cases["%s_k%d_%dto%d" % (tag, k, cin, cout)] = (n, h, w, cin, cout, k)
                    i += 1
    return cases


GRID = _grid()
# name -> shape; the comment gives items (= n * tiles) of the weight gradients whose input has Ca padded channels
EDGES = {
    "items1":   (1, 16, 16, 16, 8, 3),
    "items2":   (1, 16, 32, 3, 16, 3),        # two tiles of one image
    "items3":   (3, 16, 16, 16, 16, 3),
    "ca16_511": (73, 16, 112, 16, 8, 3),      # 2 * cap = 512 for Ca = 16
    "ca16_512": (128, 32, 32, 8, 16, 3),
    "ca16_513": (57, 48, 48, 16, 16, 3),
    "ca32_255": (85, 16, 48, 32, 8, 3),       # 2 * cap = 256 for Ca = 32
    "ca32_256": (64, 32, 32, 24, 16, 3),
    "ca32_258": (129, 16, 32, 32, 16, 3),
    "ca64_127": (127, 16, 16, 64, 8, 3),      # 2 * cap = 128 for Ca = 64
    "ca64_128": (32, 32, 32, 48, 16, 3),
    "ca64_129": (43, 16, 48, 64, 16, 3),
    "n256":     (256, 16, 16, 16, 16, 3),
    "map256":   (1, 256, 256, 16, 16, 3),     # 16 tiles in a row and in a column
}
BLOCKS = dict(GRID, **EDGES)

# the float share: six shapes that cover k in {3, 5} x NCO in {1, 2, 4}, all with a 1x1 shortcut, in all four kinds, and the longest
# chain the table has (ca64_129: workgroup 0 of g_w0 adds three tiles) on the two kinds that stress a chain
_FLOAT_SHAPES = ("r_k3_48to3", "r_k3_31to17", "r_k3_24to40", "r_k5_24to8", "p_k5_64to32", "r_k5_33to40")
FLOAT = {"f_%s_%s" % (nm, kind): (nm, kind) for nm in _FLOAT_SHAPES for kind in KINDS}
FLOAT.update({"f_ca64_129_%s" % kind: ("ca64_129", kind) for kind in ("randn", "positive")})

MASK_EDGES = {"me_k3": (2, 16, 32, 8, 24, 3), "me_k5": (3, 16, 16, 17, 17, 5)}

# name -> (n, h, w, cin, [(cout, k), ...], pool)
TRUNKS = {
    "one_k5":      (1, 16, 16, 3, [(17, 5)], 1),
    "wide_pool63": (2, 32, 16, 15, [(33, 3), (63, 5)], 1),                       # a pool behind a 64-padded ragged block
    "narrow3":     (3, 16, 32, 63, [(40, 3), (24, 5), (8, 3)], 0),
    "wide_pool49": (1, 48, 32, 8, [(17, 3), (31, 3), (48, 5), (49, 3)], 1),
    "mixed5":      (2, 16, 16, 33, [(33, 3), (31, 3), (31, 5), (15, 3), (1, 3)], 0),
    "six_256":     (1, 16, 256, 24, [(24, 3), (24, 5), (17, 3), (17, 3), (40, 3), (40, 3)], 1),
    "seven_wide":  (2, 16, 32, 1, [(3, 3), (8, 3), (15, 3), (17, 3), (24, 3), (40, 3), (63, 3)], 1),
    "eight_id":    (2, 16, 32, 16, [(16, 3)] * 8, 1),
    "eight_narrow": (1, 32, 16, 48, [(48, 3), (40, 5), (33, 3), (31, 3), (24, 5), (17, 3), (15, 3), (8, 3)], 0),
    "two_k5k5":    (3, 16, 16, 49, [(24, 5), (48, 5)], 1),
    "four_updown": (2, 48, 32, 31, [(63, 3), (15, 3), (33, 3), (3, 3)], 0),
    "three_n1":    (1, 32, 16, 40, [(40, 3), (40, 3), (17, 5)], 0),
    "five_pool":   (3, 16, 16, 17, [(8, 3), (24, 3), (24, 3), (33, 5), (33, 3)], 1),
    "sub_base":    (2, 16, 16, 8, [(17, 3), (17, 5)], 1),                        # the subnormal trunk, unscaled
}
SUBNORMAL_TRUNK = "sub_base"
TRUNK_FLOAT = ("eight_narrow", "wide_pool63", "six_256", "eight_id")      # float twins: trunk == chain of block calls
# the small k = 5 cells with NCO 1 and 2 (16x16, 32x16, 16x32) and a ragged k = 3 cell
IN_GOLDEN_BLOCKS = ("r_k5_1to17", "p_k5_64to16", "p_k5_16to16", "p_k5_64to32", "r_k3_24to1")
IN_GOLDEN_TRUNKS = ("eight_id",)
NGROUPS = 10                   # tests/test_gpu_grad_sweep.py runs the block cases in this many tests: group g is list(BLOCKS)[g::NGROUPS]


def _seed(name):
    return 20233 + sum((i + 1) * ord(ch) for i, ch in enumerate(name))


def _shape_of(name):
    return BLOCKS[name] if name in BLOCKS else MASK_EDGES[name]


def make_block(name, kind="exact"):
    """-> dict(shape, x, w0, w2, wsc or None, g_out) as float32 numpy arrays; for a MASK_EDGES case also the caller's t and out."""
    n, h, w, cin, cout, k = shape = _shape_of(name)
    g = torch.Generator().manual_seed(_seed(name + "/" + kind))
    ri = lambda lo, hi, *s: torch.randint(lo, hi + 1, s, generator=g).to(torch.float32).numpy()
    rn = lambda scale, *s: (torch.randn(s, generator=g, dtype=torch.float64) * scale).to(torch.float32).numpy()
    sign = lambda *s: 2 * ri(0, 1, *s) - 1

    def logu(lo, hi, *s):
        return (2.0 ** (lo + (hi - lo) * torch.rand(s, generator=g, dtype=torch.float64))).to(torch.float32).numpy()

    sx, sg = (n, cin, h, w), (n, cout, h, w)
    if kind == "exact":
        c = {"x": ri(-2, 2, *sx), "w0": ri(-1, 1, cout, cin, k, k), "w2": ri(-1, 1, cout, cout, k, k)}
        c["wsc"] = ri(-1, 1, cout, cin) if cin != cout else None
        c["g_out"] = ri(-1, 1, *sg)
    else:
        c = {"w0": rn((cin * k * k) ** -0.5, cout, cin, k, k), "w2": rn((cout * k * k) ** -0.5, cout, cout, k, k)}
        c["wsc"] = rn(cin ** -0.5, cout, cin) if cin != cout else None
        if kind == "randn":
            c["x"], c["g_out"] = rn(1.0, *sx), rn(1.0, *sg)
        elif kind == "positive":
            c["x"], c["g_out"] = logu(-6, 6, *sx), logu(-6, 6, *sg)
        elif kind == "wide":
            for key, s in (("x", sx), ("g_out", sg)):
                c[key] = logu(-20, 8, *s) * sign(*s) * (ri(0, 3, *s) > 0)
        elif kind == "border":
            m = np.zeros((h, w), np.float32)
            m[:2], m[-2:], m[:, :2], m[:, -2:] = 1, 1, 1, 1
            c["x"], c["g_out"] = rn(1.0, *sx) * m, rn(1.0, *sg) * m
        else:
            raise KeyError(kind)
    c["shape"] = shape
    if name in MASK_EDGES:
        values = np.array([-SUB, -0.0, 0.0, SUB, 2 * SUB], np.float32)
        c["t"], c["out"] = values[ri(0, 4, *sg).astype(np.int64)], values[ri(0, 4, *sg).astype(np.int64)]
    return c


def make_trunk(name, kind="exact"):
    """-> trunk_cases.make_case of the shape: kind "exact": its sparse +-1 scheme, "float": normal values."""
    return T.make_case(TRUNKS[name], _seed(name + "/" + kind), kind == "exact")


def scaled_trunk(c, s=SUB):
    """The case with x times s (a power of two).  Its restatement is scaled_restatement() of the unscaled one."""
    return dict(c, x=(np.asarray(c["x"], np.float64) * s).astype(np.float32))


def scaled_restatement(flat, s=SUB):
    """flat restatement of a trunk -> that of the trunk with x times s: activations and weight gradients scale, g_x does not."""
    return {k: v if k == "g_x" else v * s for k, v in flat.items()}


# ---- the dispatch of the training kernels, restated: a pure function of the shape
def wgrad_np(n, h, w, ca):
    """conv_wgrad.hip wgrad_np -> (items, NP): the work items of a weight gradient and the number of partial sums."""
    items, cap = n * (h // 16) * (w // 16), 256 // (ca // 16)
    return items, min((items + 1) // 2, cap)


def wgrads(shape):
    """The weight gradients of a block -> [(output, K, NCO, CB, items, NP)]."""
    n, h, w, cin, cout, k = shape
    r = [("g_w2", k, pad(cout) // 16, pad(cout) // 16) + wgrad_np(n, h, w, pad(cout)),
         ("g_w0", k, pad(cout) // 16, pad(cin) // 16) + wgrad_np(n, h, w, pad(cin))]
    if cin != cout:
        r.append(("g_wsc", 1, pad(cout) // 16, pad(cin) // 16) + wgrad_np(n, h, w, pad(cin)))
    return r


# the kernels of conv_wgrad.hip and trunk_glue.hip in libpmp_hip.so: tests/test_grad_cases_cpu.py holds this against the library's symbols
INSTANTIATIONS = (["wgrad_partial_kernel<%d,%d>" % (k, nco) for k in (1, 3, 5) for nco in (1, 2, 4)] +
                  ["blocked_relu_kernel<1>", "blocked_relu_kernel<2>", "grad_to_blocked_kernel<0>", "grad_to_blocked_kernel<1>",
                   "wgrad_reduce_kernel", "dense_to_blocked_kernel", "blocked_to_dense_kernel", "pack_mfma_kernel", "pool_to_dense_kernel"])
SYMBOL_PATTERN = (r"_ZN3pmp\d+(wgrad_partial_kernel|blocked_relu_kernel|grad_to_blocked_kernel|wgrad_reduce_kernel|dense_to_blocked_kernel|"
                  r"blocked_to_dense_kernel|pack_mfma_kernel|pool_to_dense_kernel)(?:I((?:L[ib]\d+E)+)E)?")


def block_kernels(shape):
    """The kernels of INSTANTIATIONS a pmp_resblock_forward + _backward of this shape launches."""
    ks = {"dense_to_blocked_kernel", "blocked_to_dense_kernel", "pack_mfma_kernel", "wgrad_reduce_kernel", "blocked_relu_kernel<2>"}
    return ks | {"wgrad_partial_kernel<%d,%d>" % (k, nco) for _, k, nco, _, _, _ in wgrads(shape)}


def trunk_kernels(shape):
    n, h, w, cin, blocks, pool = shape
    ks = {"dense_to_blocked_kernel", "blocked_to_dense_kernel", "pack_mfma_kernel", "wgrad_reduce_kernel", "blocked_relu_kernel<2>",
          "grad_to_blocked_kernel<%d>" % pool}
    if pool:
        ks.add("pool_to_dense_kernel")
    if len(blocks) > 1:
        ks.add("blocked_relu_kernel<1>")
    for ci, co, k in T.block_shapes(shape):
        ks |= {"wgrad_partial_kernel<%d,%d>" % (kk, nco) for _, kk, nco, _, _, _ in wgrads((n, h, w, ci, co, k))}
    return ks


# ---- float64 references with their per-element bounds
def _d(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, np.float64))


def float_reference(c, c_wgrad=C_WGRAD):
    """A float case -> (t32, out32, ref, bound, parts).  t32, out32: the float32 roundings of the float64 forward, which the backward
    pass is given; ref, bound: float64 numpy arrays over resblock_cases.OUTPUTS (None where absent); parts: the operands of the three
    weight gradients, name -> (a, g, A), for emulate_wgrad.  The values are resblock_cases.forward's and backward's
    (tests/test_grad_cases_cpu.py); they are recomputed here only because the bounds need gu and gt, which backward() keeps."""
    x, w0, w2, g = _d(c["x"]), _d(c["w0"]), _d(c["w2"]), _d(c["g_out"])
    wsc4 = None if c["wsc"] is None else _d(c["wsc"]).reshape(c["wsc"].shape[0], c["wsc"].shape[1], 1, 1)
    p = w0.shape[2] // 2
    conv = lambda a, w, pp=p: F.conv2d(a, w, padding=pp)
    convt = lambda a, w, pp=p: F.conv_transpose2d(a, w, padding=pp)
    wg = lambda a, w, gg, pp=p: torch.nn.grad.conv2d_weight(a, w.shape, gg, padding=pp)
    rnd = lambda c_, A, ref, P=0.0: c_ * EPS * A + R_STORE * ref.abs() + P
    ref, bnd = {}, {}
    # forward
    t = F.relu(conv(x, w0))
    ref["t"], bnd["t"] = t, rnd(C_CONV, conv(x.abs(), w0.abs()), t)
    sc, asc = (x, x.abs()) if wsc4 is None else (conv(x, wsc4, 0), conv(x.abs(), wsc4.abs(), 0))
    out = F.relu(conv(t, w2) + sc)
    ref["out"], bnd["out"] = out, rnd(C_CONV, conv(t, w2.abs()) + asc, out, conv(bnd["t"], w2.abs()))
    # backward, from the float32 roundings of t and out
    t32, out32 = K.as_f32(t.numpy()), K.as_f32(out.numpy())
    tt, zero = _d(t32), torch.zeros((), dtype=torch.float64)
    gu = torch.where(_d(out32) > 0, g, zero)
    parts = {"g_w2": (t32, gu.numpy().astype(np.float32), wg(tt, w2, gu.abs()))}
    ref["g_w2"] = wg(tt, w2, gu)
    bnd["g_w2"] = rnd(c_wgrad, parts["g_w2"][2], ref["g_w2"])
    ref["g_wsc"] = bnd["g_wsc"] = None
    if wsc4 is not None:
        parts["g_wsc"] = (c["x"], parts["g_w2"][1], wg(x.abs(), wsc4, gu.abs(), 0).reshape(c["wsc"].shape))
        ref["g_wsc"] = wg(x, wsc4, gu, 0).reshape(c["wsc"].shape)
        bnd["g_wsc"] = rnd(c_wgrad, parts["g_wsc"][2], ref["g_wsc"])
    m = tt > 0
    gt = torch.where(m, convt(gu, w2), zero)
    b_gt = torch.where(m, rnd(C_CONV, convt(gu.abs(), w2.abs()), gt), zero)
    ref["g_w0"] = wg(x, w0, gt)
    bnd["g_w0"] = rnd(c_wgrad, wg(x.abs(), w0, gt.abs()), ref["g_w0"], wg(x.abs(), w0, b_gt))
    a_gx = convt(gt.abs(), w0.abs()) + (gu.abs() if wsc4 is None else convt(gu.abs(), wsc4.abs(), 0))
    ref["g_x"] = convt(gt, w0) + (gu if wsc4 is None else convt(gu, wsc4, 0))
    bnd["g_x"] = rnd(C_CONV, a_gx, ref["g_x"], convt(b_gt, w0.abs()))
    # g_w0 for the emulation: the operation on the float32 gt a kernel would hand it, against float64 on the same operands
    gt32 = K.as_f32(gt.numpy())
    parts["g_w0"] = (c["x"], gt32, wg(x.abs(), w0, _d(gt32).abs()))
    num = lambda d: {k: None if v is None else v.numpy() for k, v in d.items()}
    return t32, out32, num(ref), num(bnd), {k: (a, gg, A.numpy()) for k, (a, gg, A) in parts.items()}


def wgrad64(a, g, k):
    """The float64 weight gradient of float32 operands a [n,ci,h,w] and g [n,co,h,w] -> [co,ci,k,k]."""
    return torch.nn.grad.conv2d_weight(_d(a), (g.shape[1], a.shape[1], k, k), _d(g), padding=k // 2).numpy()


def emulate_wgrad(a, g, k):
    """conv_wgrad.hip's order of summation in float32 on the CPU -> float32 [co,ci,k,k].  Workgroup p of NP adds the items p, p + NP,
    ... (an item: one 16x16 tile of one image, tiles in row order), each pixel by pixel in row order, acc = float32(acc + g * a) with
    the product exact (a float64 product of float32 operands: what a fused multiply-add rounds); the NP partial sums are then added in
    float32 in the order 0 .. NP-1.  The order of the four products inside one MFMA is the hardware's; here they follow the pixels."""
    n, ci, h, w = a.shape
    co, p = g.shape[1], k // 2
    items, NP = wgrad_np(n, h, w, pad(ci))
    tiles_x, tiles = w // 16, (w // 16) * (h // 16)
    ap = F.pad(_d(a), (p, p, p, p))
    gd = _d(g)
    acc = torch.zeros((NP, co, ci, k, k), dtype=torch.float32)
    for first in range(0, items, NP):
        its = list(range(first, min(first + NP, items)))
        at = torch.zeros((NP, ci, 16 + 2 * p, 16 + 2 * p), dtype=torch.float64)
        gt = torch.zeros((NP, co, 16, 16), dtype=torch.float64)          # a workgroup without an item in this round adds zeros
        for q, it in enumerate(its):
            nn, tt = divmod(it, tiles)
            ty, tx = divmod(tt, tiles_x)
            at[q] = ap[nn, :, ty * 16:ty * 16 + 16 + 2 * p, tx * 16:tx * 16 + 16 + 2 * p]
            gt[q] = gd[nn, :, ty * 16:ty * 16 + 16, tx * 16:tx * 16 + 16]
        for y in range(16):
            for x in range(16):
                prod = gt[:, :, None, None, None, y, x] * at[:, None, :, y:y + k, x:x + k]
                acc = (acc.double() + prod).float()
    s = acc[0]
    for q in range(1, NP):
        s = s + acc[q]
    return s.numpy()


# ---- the mask-edge cases: backward only, from the caller's t and out
def mask_edges_reference(c):
    """-> (float64 backward of the case on its own t and out, the largest sum of |terms| of any output element in units of that
    output's grid: 2^-149 for g_w2, 1 for the others; |gt| enters as the sum of ITS |terms|, an upper bound).  Below 2^24 every partial
    sum in any order is exact in float32, the subnormal ones included: integer multiples of 2^-149 below 2^-125."""
    r = K.backward(c["x"], c["t"], c["out"], c["w0"], c["w2"], c["wsc"], c["g_out"])
    x, t, out, w0, w2, g = (_d(np.abs(c[k])) for k in ("x", "t", "out", "w0", "w2", "g_out"))
    wsc4 = None if c["wsc"] is None else _d(np.abs(c["wsc"])).reshape(c["wsc"].shape[0], c["wsc"].shape[1], 1, 1)
    p = w0.shape[2] // 2
    zero = torch.zeros((), dtype=torch.float64)
    wg = lambda a, w, gg, pp=p: torch.nn.grad.conv2d_weight(a, w.shape, gg, padding=pp)
    gu = torch.where(_d(c["out"]) > 0, g, zero)
    gt = torch.where(_d(c["t"]) > 0, F.conv_transpose2d(gu, w2, padding=p), zero)
    sums = [wg(t, w2, gu) / SUB, gt, wg(x, w0, gt), F.conv_transpose2d(gt, w0, padding=p) + (gu if wsc4 is None else F.conv_transpose2d(gu, wsc4))]
    if wsc4 is not None:
        sums.append(wg(x, wsc4, gu, 0))
    return r, max(float(v.max()) for v in sums)


@functools.lru_cache(maxsize=None)
def trunk_exact(name):
    """-> (case, float64 restatement, flat); computed once, never changed."""
    c = make_trunk(name)
    return c, T.flat(T.restate(c))
