"""The cases of the divergence guard (include/pmp.h, TRAINING STEP: pmp_grad_guard_device, pmp_adam_step_guarded_device) and its
restatement in numpy, for test_guard_cases_cpu.py and test_gpu_grad_guard.py.

census(): the header's ORDER OF THE CENSUS in float64, lane by lane and level by level.  Tensor i is cut into tiles of 4096 elements,
numbered through the tensors in the order given.  In a tile lane l of 256 adds the squares of its elements l, l + 256, ..., l + 256*15
that exist and are finite, in ascending order from +0.0; then a[l] += a[l + h] for l < h, h = 128, 64, ..., 1, and a[0] is the tile's
partial.  One more round of the same shape adds the partials: lane l takes partials l, l + 256, ..., then the tree.  An element that
does not exist or is not finite adds nothing; adding +0.0 in its place gives the same bits, because every sum here is >= +0.0.
record(): the header's record rule.  counters(): the running counters after a sequence of records.
The tables: counts drawn from COUNTS, one tensor and 97 (two launches of PMP_ADAM_TABLE = 96 entries: the tile numbering crosses the
table), values sign * 10^u, u uniform in [-30, 18], so that the squares span 1e-60 .. 1e36 and a float32 sum would visibly differ, and
PLANTS: where NaN and inf are put.  A plain module."""
import math

import numpy as np

TILE, LANES = 4096, 256
COUNTS = (1, 3, 255, 256, 257, 4095, 4096, 4097, 2 * 4096 + 1)
ACTION_SKIP, ACTION_CLIP = 1, 2
STATE_KEYS = ("steps", "skipped", "clipped", "run", "max_run", "max_norm")


def _lanes_then_tree(rows):
    """rows float64[k][256], row j holding what the lanes add j-th -> a[0] behind the lanes' sums and the tree"""
    a = np.zeros(LANES, np.float64)                      # from +0.0
    for row in rows:                                     # ascending
        a = a + row
    h = LANES // 2
    while h >= 1:
        a[:h] = a[:h] + a[h:2 * h]                       # a[l] += a[l + h] for l < h
        h //= 2
    return a[0]


def census(tensors):
    """tensors: float32 arrays in the call's order -> (sumsq float64, nonfinite int, the tiles' partials float64[tiles])"""
    partials, nonfinite = [], 0
    for t in tensors:
        t = np.asarray(t, np.float32).ravel()
        for base in range(0, t.size, TILE):
            tile = t[base:base + TILE]
            ok = np.isfinite(tile)
            nonfinite += int((~ok).sum())
            d = np.where(ok, tile, np.float32(0)).astype(np.float64)
            sq = np.zeros(TILE, np.float64)
            sq[:tile.size] = d * d                       # exact: 24 bits squared
            partials.append(_lanes_then_tree(sq.reshape(TILE // LANES, LANES)))      # element l + 256 j is row j, lane l
    p = np.zeros(-(-len(partials) // LANES) * LANES, np.float64)
    p[:len(partials)] = partials
    return float(_lanes_then_tree(p.reshape(-1, LANES))), nonfinite, np.array(partials, np.float64)


def record(sumsq, nonfinite, max_norm=0.0, skip_nonfinite=False):
    """-> pmp_guard_record as a dict"""
    norm = float(np.sqrt(np.float64(sumsq)))
    c = np.float64(max_norm) / (np.float64(norm) + np.float64(1e-6))
    coef = np.float32(c) if max_norm > 0 and c < 1 else np.float32(1.0)
    action = (ACTION_SKIP if skip_nonfinite and nonfinite > 0 else 0) | (ACTION_CLIP if coef < np.float32(1.0) else 0)
    return {"sumsq": float(sumsq), "norm": norm, "nonfinite": int(nonfinite), "coef": coef, "action": action}


def counters(records, start=None):
    """pmp_guard_state after grad_guard calls that wrote `records`, in order, from `start` (zeros)"""
    s = dict(start or {"steps": 0, "skipped": 0, "clipped": 0, "run": 0, "max_run": 0, "max_norm": 0.0})
    for r in records:
        s["steps"] += 1
        if r["action"] & ACTION_SKIP:
            s["skipped"] += 1
            s["run"] += 1
            s["max_run"] = max(s["max_run"], s["run"])
        else:
            s["run"] = 0
            if r["action"] & ACTION_CLIP:
                s["clipped"] += 1
        s["max_norm"] = max(s["max_norm"], r["norm"])
    return s


def exact_sumsq(tensors):
    """math.fsum of the exact squares of the finite elements: the correctly rounded sum"""
    out = []
    for t in tensors:
        d = np.asarray(t, np.float32).ravel().astype(np.float64)
        out.append((d[np.isfinite(d)] ** 2).tolist())
    return math.fsum(v for part in out for v in part)


# ---- the tables
def _values(rng, n):
    return (rng.choice([-1.0, 1.0], n) * 10.0 ** rng.uniform(-30.0, 18.0, n)).astype(np.float32)


TABLES = {"one_1": [1], "one_4097": [4097], "one_8193": [2 * 4096 + 1], "nine": list(COUNTS),
          "ninety_seven": [COUNTS[(5 * i + 3) % len(COUNTS)] for i in range(96)] + [4097]}

# name -> [(tensor by its position from the END of the table, element, value)]; the tables that take plants end in a tensor of 4097
# or 8193 elements, and "nine" has its 4096 at position -3
NAN, INF = float("nan"), float("inf")
PLANTS = {"none": [],
          "first_of_a_tile": [(-1, 4096, NAN)],
          "last_of_a_tile_lane_255s_last_slot": [(-1, 255 + 256 * 15, INF)],
          "end_of_the_ragged_tail": [(-1, -1, -INF)],
          "mixed": [(-1, 0, NAN), (-1, 4095, INF), (-1, 4096, -INF), (-1, 17, -INF), (-1, 300, NAN)]}


def table(name, plant="none", seed=0):
    """-> the float32 tensors of table `name` with PLANTS[plant] put in"""
    rng = np.random.default_rng(1000 + seed + sum(map(ord, name)))
    ts = [_values(rng, n) for n in TABLES[name]]
    for pos, el, v in PLANTS[plant]:
        assert ts[pos].size >= 4097
        ts[pos][el] = v
    return ts


CASES = [(name, plant) for name in TABLES for plant in PLANTS if plant == "none" or TABLES[name][-1] >= 4097]

# the record rule's settings a case is run under: (max_norm, skip_nonfinite)
RULES = ((0.0, False), (0.0, True), (1.0, True), (1e30, False))
