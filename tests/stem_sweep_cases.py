"""The stem's sweep (include/pmp.h: pmp_stem_*; csrc/stem_train.hip) over every shape the header accepts: the table only, on the float64
machinery of tests/stem_cases.py (make_case, restate, backward, emulate_*, worst_partial_sum).  tests/test_stem_sweep_cpu.py asserts
the table's reach and fitness, tests/test_gpu_stem_sweep.py runs it.  One kernel set serves every (cin, k, split) with its geometry
read at run time; stem_cases holds six of the sixteen triples.

EXACT cases, name -> (n, h, w, cin, k, split), values as in stem_cases (pixels 0..255, the QT channel of a split stem 0..3, +-1
weights, biases -3..3, g_y in {-1, 0, 1}) and worst_partial_sum() below 2^24: bit for bit in any order.
  one_c<cin>k<k>s<split>   all sixteen triples on one tile whose whole halo is padding
  two_c<cin>k<k>s<split>   all sixteen at (2, 32, 48): 12 items on NP = 6 - every workgroup adds two items of different images, halos
                           from real neighbours on both axes.  NT = ceil((cin k k + 1) / 16) takes 2, 4, 5, 6, 7, 11, 16 and 21
  x256, luma256, tall, wide, n256   sides and n at the header's 256: the input gradient's seventeenth tile row / column of k/2 lines
  parts4, parts5, cap_luma, cap_wide, four   (g_y sparse, one pixel in sixteen) the partition: 4 and 5 items; NP = 512 with NT = 11
                           (the trainer's luma MTT stem; workgroups 0..15 add three items) and with NT = 21 on exactly 2 * 512 items;
                           1540 items, of which workgroups 0..3 add four
MASK_EDGES: the backward pass alone, GIVEN a y drawn from {-2^-149, -0, +0, 2^-149, 2^-126, 1}; reference backward(c, y) on that y.
TINY: an exact case scaled by 2^-149, a power of two - in x and the biases (x_tiny: y and every g_w are the unscaled integers times
2^-149, g_x and g_b stay integers; forward and backward run on the GPU, so the mask sees subnormals the forward kernel made itself) or
in g_y (g_tiny: g_x, every g_w and g_b).  Every scaled value is an integer below 2^24 in units of 2^-149, which float32 holds exactly
on both sides of 2^-126: still bit for bit in any order, provided no kernel flushes.

FLOAT cases, name -> (shape name, kind of stem_cases.KINDS), shapes in FLOAT_SHAPES: the longest and the shortest forward chain
(R = 324 and 25), and f_parts with 128 items on NP = 64 - a real second-stage chain, where stem_cases' float cases have NP = 2 and 3.
BOUND per element, stem_cases' form: |gpu - ref64| <= c * 2^-24 * A + 2^-23 * |ref64|.  c per kernel is the larger of stem_cases'
constant and twice what the float32 emulation of the documented order of additions (stem_cases.emulate_*, on the CPU) reaches on THIS
table, in units of 2^-24 * A:
    forward          emulated 7.85  (7.843: y of f_parts_positive; 3.0-6.7 on the others)                 -> C_FWD   = 15.7   (stem_cases: 14)
    weight gradient  emulated 13.27 (13.262: g_w0 of f_m39_positive, 1024 pixels of one sign in two workgroups; 12.94 on
                                     f_q49_positive, 12.35 on f_m15_positive, 8.1 on f_parts_positive, whose 64 partial sums
                                     add two items each; 0.2-2.6 on randn and pixels; the bias gradients 0.1-9.5)   -> C_WGRAD = 26.54  (stem_cases: 25)
    input gradient   emulated 10.80 (10.798: g_x of f_parts_positive, one chain of 2592 terms; 8.5 on f_m39_positive and
                                     f_m15_positive, 2.4-6.2 on the others)                                       -> C_DGRAD = 21.6   (stem_cases: 15.4)
(tests/test_stem_sweep_cpu.py prints the figures under `pytest -s` and asserts that the emulation stays within half of each bound.)
Largest |gpu - ref64| / bound on an MI355X (tests/test_gpu_stem_sweep.py prints them under `pytest -s`), GPU_RATIOS below:
    stem_forward_kernel 0.474 (f_parts_positive; 0.19-0.40 on the others)     stem_wgrad_kernel + stem_reduce_kernel 0.465
    (f_m39_positive; 0.453 on f_q49_positive, 0.433 on f_m15_positive, 0.02-0.31 on the others)     stem_dgrad_kernel 0.480
    (f_parts_positive; 0.383 on f_m39_positive, 0.11-0.37 on the others): below half of each bound, where the emulation on the
    same three cases is at half by construction.
"""
import functools

import numpy as np

import stem_cases as S

TRIPLES = [(cin, k, split) for cin in (1, 2, 3, 4) for k in (5, 9) for split in (0, 1)]
ONE, TWO = (1, 16, 16), (2, 32, 48)


def _tname(prefix, t):
    return "%s_c%dk%ds%d" % ((prefix,) + t)


EXACT = {_tname("one", t): ONE + t for t in TRIPLES}
EXACT.update({_tname("two", t): TWO + t for t in TRIPLES})
EXTENTS = {
    "x256":    (1, 256, 256, 1, 5, 0),
    "luma256": (1, 256, 256, 2, 9, 1),
    "tall":    (1, 256, 16, 3, 9, 1),
    "wide":    (1, 16, 256, 4, 9, 1),
    "n256":    (256, 16, 16, 3, 9, 1),
}
PARTITION = {                                      # name -> shape; (items, NP) in PROMISED
    "parts4":   (1, 32, 32, 4, 9, 1),
    "parts5":   (1, 16, 80, 4, 9, 1),
    "cap_luma": (65, 64, 64, 2, 9, 1),
    "cap_wide": (64, 64, 64, 4, 9, 1),
    "four":     (55, 64, 112, 1, 5, 0),
}
PROMISED = {"parts4": (4, 2), "parts5": (5, 3), "cap_luma": (1040, 512), "cap_wide": (1024, 512), "four": (1540, 512)}
EXACT.update(EXTENTS)
EXACT.update(PARTITION)
SPARSE = tuple(PARTITION)

MASK_EDGES = {"mask_m29": (2, 32, 48, 2, 9, 1), "mask_q35": (2, 16, 32, 3, 5, 0)}
MASK_VALUES = np.array([-2.0 ** -149, -0.0, 0.0, 2.0 ** -149, 2.0 ** -126, 1.0], np.float32)
TINY = {"tiny_m29": (1, 16, 32, 2, 9, 1), "tiny_q35": (1, 16, 16, 3, 5, 0)}
TINY_SCALE = 2.0 ** -149
ARENA = {"a_q15": (1, 16, 32, 1, 5, 0), "a_m45": (1, 32, 16, 4, 5, 1), "a_q29": (2, 16, 16, 2, 9, 0), "a_m49": (1, 16, 32, 4, 9, 1),
         "a_m39": (1, 32, 32, 3, 9, 1)}
STEM_PY = {"py_m29": (2, 32, 16, 2, 9, 1), "py_q35": (2, 16, 32, 3, 5, 0)}

FLOAT_SHAPES = {
    "f_q49":   (2, 32, 16, 4, 9, 0),
    "f_m15":   (3, 16, 32, 1, 5, 1),
    "f_m39":   (1, 32, 32, 3, 9, 1),
    "f_q25":   (2, 16, 48, 2, 5, 0),
    "f_parts": (8, 64, 64, 2, 9, 1),
}
FLOAT = {"%s_%s" % (nm, kind): (nm, kind) for nm in FLOAT_SHAPES for kind in S.KINDS}
C_FWD_EMULATED, C_WGRAD_EMULATED, C_DGRAD_EMULATED = 7.85, 13.27, 10.80          # on this table: the docstring says where
C_FWD, C_WGRAD, C_DGRAD = max(S.C_FWD, 2 * C_FWD_EMULATED), max(S.C_WGRAD, 2 * C_WGRAD_EMULATED), max(S.C_DGRAD, 2 * C_DGRAD_EMULATED)
C_OF = {"forward": C_FWD, "wgrad": C_WGRAD, "dgrad": C_DGRAD}
GPU_RATIOS = {"forward": 0.474, "wgrad": 0.465, "dgrad": 0.480}      # largest |gpu - ref64| / bound measured on an MI355X


def nt(shape):
    """csrc/stem_train.hip stem_nt: the weight gradient's column tiles, R reduction indices and the bias column."""
    return (shape[3] * shape[4] * shape[4] + 1 + 15) // 16


def items_per_workgroup(shape):
    """-> (most, fewest) items a workgroup of the weight gradient adds: workgroup q takes q, q + NP, ..."""
    items, NP = S.stem_np(shape)
    return -(-items // NP), items // NP


@functools.lru_cache(maxsize=None)
def exact(name):
    """-> (case, the float64 restatement as the float32 a kernel must produce); computed once, never changed."""
    c = S.make_case(name, shape=EXACT[name], sparse=name in SPARSE)
    return c, {k: S.as_f32(v) for k, v in S.flat(S.restate(c)).items()}


# ---- masks on the edge of `> 0`
@functools.lru_cache(maxsize=None)
def mask_edges(name):
    """-> (case, y, want): y float32 of MASK_VALUES, every one of them in every output channel; want from backward(c, y) in float64."""
    c = S.make_case(name, shape=MASK_EDGES[name])
    n, h, w = c["shape"][:3]
    rng = np.random.RandomState(S._seed(name) % 2 ** 31)
    y = MASK_VALUES[rng.randint(0, len(MASK_VALUES), (n, 32, h, w))]
    want = {k: S.as_f32(v) for k, v in S.flat(dict(S.backward(c, y), y=y)).items()}
    want["y"] = y                                  # given, not computed: it keeps its -0
    return c, y, want


# ---- an exact case times 2^-149
def scaled(c, which):
    """x_tiny: x and the biases times 2^-149; g_tiny: g_y.  Exact in float32: every value is an integer below 2^24 in units of 2^-149."""
    f = np.float32(TINY_SCALE)
    c = dict(c)
    if which == "x_tiny":
        c["x"], c["b"] = c["x"] * f, [b * f for b in c["b"]]
    elif which == "g_tiny":
        c["g_y"] = c["g_y"] * f
    else:
        raise KeyError(which)
    return c


def scaled_outputs(c, which):
    """The outputs that carry the factor 2^-149."""
    gw = ["g_w%d" % j for j in range(len(c["w"]))]
    return ["y"] + gw if which == "x_tiny" else ["g_x"] + gw + ["g_b%d" % j for j in range(len(c["w"]))]


@functools.lru_cache(maxsize=None)
def tiny(name, which):
    """-> (the scaled case, want, the unscaled float64 restatement): want is the float64 restatement OF THE SCALED CASE - float64 holds
    integers times 2^-149 and their sums exactly - as float32."""
    base = S.make_case(name, shape=TINY[name])
    c = scaled(base, which)
    want = {k: S.as_f32(v) for k, v in S.flat(S.restate(c)).items()}
    return c, want, S.flat(S.restate(base))


# ---- float cases
def KERNEL_OF(key):
    return S.KERNEL_OF(key)


@functools.lru_cache(maxsize=None)
def float_reference(name):
    """stem_cases.float_reference with this table's shapes and constants -> (case, y32, ref, bound, A)."""
    nm, kind = FLOAT[name]
    c = S.make_case(nm, kind, shape=FLOAT_SHAPES[nm])
    y = S.forward(c)
    y32 = S.as_f32(y)
    ref = S.flat(dict(S.backward(c, y32), y=y))
    A = S.flat(dict(S.backward(c, y32, absolute=True), y=S.forward(c, absolute=True)))
    bound = {key: C_OF[KERNEL_OF(key)] * S.EPS * A[key] + S.R_STORE * np.abs(ref[key]) for key in ref}
    return c, y32, ref, bound, A


def units(got, ref, A):
    """max |got - ref| / (2^-24 A): the figure the constants are made of."""
    d = np.abs(np.asarray(got, np.float64) - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        return float(np.where(d == 0, 0.0, d / (S.EPS * A)).max())
