"""Inputs behind tests/golden/g10_m2p_params.npz: Map2Partition with other thresholds (include/pmp.h: pmp_partition_params).

The fixture holds outputs only.  Its inputs are slices of G3, G3b and G9 plus "probe" triples whose direction cells sit at
float32(thd) and its float32 neighbours (probe_triples), so that tools/gen_golden_m2p_params.py (which runs the
reference on them) and the tests (which run the library on them) see the same numbers.  Not a test module: no test_ prefix."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

DEFAULT = (0.7, 0.7, 1.5, 0.3, 0.7, 0.5)            # Map2Partition.py:100 (lamb1..lamb5), :105 (thd)
# name -> (lamb1, lamb2, lamb3, lamb4, lamb5, thd)
SETS = {
    "defaults": DEFAULT,
    "ties": (0.75, 0.5, 1.0, 0.25, 0.75, 0.5),      # products that are exact integers: >= against > decides
    "early_stop": (0.5, 0.9, 2.0, 0.2, 0.8, 0.5),
    "permissive": (1.0, 0.3, 1.1, 0.5, 0.67, 0.5),
    "lamb3_0p8": (0.7, 0.7, 0.8, 0.3, 0.7, 0.5),    # lamb3 < 1: both direction tests can hold, the first one wins
    # thd sets: lamb3 chosen so that the probe triples (probe_triples) tell the semantics apart
    "thd_0p7": (0.7, 0.7, 1.0, 0.3, 0.7, 0.7),     # float32(0.7) > 0.7: a float32 compare and a double one differ
    "thd_1p0": (0.7, 0.7, 1.0, 0.3, 0.7, 1.0),
    "thd_1p5": (0.7, 0.7, 0.8, 0.3, 0.7, 1.5),     # th_round's third step zeroes every direction
}
G3B_SET = "ties"          # the set run over the G3b slice (non-finite and huge logits)
G3B_SLICE = slice(0, 650, 10)

# per chroma factor: (source, slice) of the G3 / G9 triples
G3_SLICES = (("q", slice(0, 160)), ("r", slice(0, 32)), ("a", slice(0, 54)), ("t", slice(0, 4)))
G9_SLICES = (("rand", slice(0, 40)), ("raw", slice(0, 12)))


def kw(name):
    """The set as keyword arguments named as in the reference."""
    v = SETS[name]
    return dict(zip(("lamb1", "lamb2", "lamb3", "lamb4", "lamb5", "thd"), v))


def probe_triples(thd):
    """th_round's ties: one unsplit 64x64 CU whose depth maps ask for one binary split (rounded depth 1 on all three layers), so the
    candidates are no split, BT-H and BT-V; the direction gating alone decides between them.  Layer 0 of the direction map holds `nh`
    cells (row-major first) at v in {float32(thd), its upper and its lower float32 neighbour} and -2 elsewhere (and the mirror image,
    every value negated).  With the counts chosen here the gating picks one direction when v counts as +-1 and the error sum the
    other one when it does not, so a threshold compared in double instead of float32, or th_round's thd > 1 step left out, moves the
    split.  -> (qt, bt, dire), 12 triples."""
    t = np.float32(thd)
    qt, bt, dire = [], [], []
    for nh in (140, 120):
        for v in (t, np.nextafter(t, np.float32(np.inf)), np.nextafter(t, np.float32(0))):
            for sign in (1.0, -1.0):
                d = np.zeros((3, 256), np.float32)
                d[0, :nh] = v
                d[0, nh:] = -2.0
                qt.append(np.zeros((8, 8), np.float32))
                bt.append(np.ones((3, 16, 16), np.float32))
                dire.append((d * np.float32(sign)).reshape(3, 16, 16))
    return np.stack(qt), np.stack(bt), np.stack(dire)


def inputs(cf, thd):
    """[(source, qt f32[n,8,8] as handed to pmp_postprocess (depth maps or raw logits), bt f32[n,3,16,16], dire)] for one chroma factor."""
    g3 = np.load(os.path.join(GOLDEN, "g3_m2p.npz"))
    g9 = np.load(os.path.join(GOLDEN, "g9_m2p_seeded.npz"))
    out = []
    for t, sl in G3_SLICES:
        qt = g3["%s_qt_cf%d" % (t, cf)][sl].astype(np.float32)
        if t == "q":
            bt = (g3["q_bt64_cf%d" % cf][sl] / 64.0).astype(np.float32)
            dire = (g3["q_dire64_cf%d" % cf][sl] / 64.0).astype(np.float32)
        else:
            bt, dire = g3["%s_bt_cf%d" % (t, cf)][sl], g3["%s_dire_cf%d" % (t, cf)][sl]
        out.append(("g3" + t, qt, bt, dire))
    for t, sl in G9_SLICES:
        out.append(("g9" + t, g9["%s_qt_cf%d" % (t, cf)][sl].astype(np.float32), g9["%s_bt_cf%d" % (t, cf)][sl],
                    g9["%s_dire_cf%d" % (t, cf)][sl]))
    out.append(("probe",) + probe_triples(thd))
    return out


def g3b_inputs(cf):
    """(qt RAW logits, bt, dire, fixed = the reference's eli_structual_error of qt) of the G3b slice."""
    g = np.load(os.path.join(GOLDEN, "g3b_m2p_range.npz"))
    return tuple(g["%s_cf%d" % (k, cf)][G3B_SLICE] for k in ("qt", "bt", "dire", "fixed"))


def expected(g10, name, source, cf):
    """(hor, ver, dout) of the fixture for one set, source and chroma factor."""
    return tuple(g10["%s_%s_%s_cf%d" % (name, source, k, cf)] for k in ("hor", "ver", "dout"))
