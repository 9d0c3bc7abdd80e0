"""Inputs behind tests/golden/g11_msbt.npz (GenMSBtMap labels, include/pmp.h: pmp_msbt_labels; the DecLib dump parser,
pmp_read_depth_dump), and a numpy restatement of GenMSBtMap.Map_to_SubMap that also defines the answer where the reference has none.

The fixture holds outputs only.  Its inputs are rebuilt here from seeds, so that tools/gen_golden_msbt.py (which runs the reference on
them) and the tests (which run the library on them) see the same bytes.  Not a test module: no test_ prefix."""
import itertools
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from pmp_vvc_tip2023_amd import synth  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "g11_msbt.npz")
BUDGET = 4096                                   # PMP_MSBT_LEAF_BUDGET
INCONSISTENT, QT_DEEP, OVER_BUDGET = 1, 2, 4    # status bits
L1, L2, L3, L4, L5 = 0.8, 1.0, 1.2, 0.2, 0.2     # GenMSBtMap.py:91


# ------------------------------------------------------------------------------------------------ label triples
def _labels(qt, bt, dire):
    """synth's float maps -> CreateDataSet's dtypes: qt u8 (already qtDepth - 1), the final MTT depth bt u8, dire i8."""
    return qt.astype(np.uint8), bt[2].astype(np.uint8), dire.astype(np.int8)


def valid_blocks(n, seed, cf):
    rng = np.random.default_rng(seed)
    out = [_labels(*synth.random_partition_maps(rng, cf)) for _ in range(n)]
    return tuple(np.stack(a) for a in zip(*out))


def noisy_blocks(n, seed, frac=0.1):
    """Valid cf-1 partitions with +-1 label noise on `frac` of the bt cells: many blocks make the reference raise."""
    qt, bt, dire = valid_blocks(n, seed, 1)
    rng = np.random.default_rng(seed + 1)
    m = rng.random(bt.shape) < frac
    d = rng.choice(np.array([-1, 1]), size=bt.shape)
    bt = np.clip(bt.astype(np.int16) + m * d, 0, 255).astype(np.uint8)
    return qt, bt, dire


def _checker():
    return np.where((np.arange(16)[:, None] + np.arange(16)[None, :]) % 2 == 0, 1, -1).astype(np.int8)


def tie_blocks(n, seed):
    """QT regions with a uniform label depth and a balanced direction map: BT-H and BT-V (or more) reach the same error; the first
    in DFS order must win."""
    rng = np.random.default_rng(seed)
    qt = np.zeros((n, 8, 8), np.uint8); bt = np.zeros((n, 16, 16), np.uint8); dire = np.zeros((n, 3, 16, 16), np.int8)
    cb = _checker()
    for i in range(n):
        depth = int(rng.integers(0, 3))
        qt[i] = depth
        s = 16 >> depth
        for r in range(0, 16, s):
            for c in range(0, 16, s):
                bt[i, r:r + s, c:c + s] = rng.integers(1, 3)
        for k in range(3):
            dire[i, k] = cb if rng.random() < 0.7 else -cb
    return qt, bt, dire


def qt_deep_blocks(n, seed):
    """Valid cf-1 partitions with one or more quadrants' qt set to 4..6: the reference leaves those regions zero."""
    qt, bt, dire = valid_blocks(n, seed, 1)
    rng = np.random.default_rng(seed + 7)
    for i in range(n):
        for qd in range(4):
            if rng.random() < 0.5 or qd == 0:
                r, c = (qd >> 1) * 4, (qd & 1) * 4
                qt[i, r:r + 4, c:c + 4] = rng.integers(4, 7)
    return qt, bt, dire


def big_tree_blocks():
    """Regions whose labels admit many splits (a uniform label depth of 2..4 and a checkerboard direction map, which dominates without
    a direction): trees of up to a few hundred leaves per region that the reference finishes."""
    qt = np.array([0, 0, 1, 2], np.uint8)[:, None, None] * np.ones((1, 8, 8), np.uint8)
    bt = np.array([2, 3, 3, 4], np.uint8)[:, None, None] * np.ones((1, 16, 16), np.uint8)
    dire = np.broadcast_to(_checker(), (4, 3, 16, 16)).copy()
    return qt, bt, dire


def over_budget_blocks():
    """32x32 regions of 8184 leaves each (cf 1; labels 3 on the left half, 4 on the right): the reference finishes them, the library
    stops at the budget (status bit 4) with the best of the first PMP_MSBT_LEAF_BUDGET leaves."""
    bt = np.full((1, 16, 16), 3, np.uint8); bt[:, :, 8:] = 4
    return np.ones((1, 8, 8), np.uint8), bt, np.broadcast_to(_checker(), (1, 3, 16, 16)).copy()


def worst_blocks(n):
    """Labels that admit every legal split in one 64x64 region: millions of leaves (cf 1), far beyond the budget."""
    qt = np.zeros((n, 8, 8), np.uint8)
    bt = np.full((n, 16, 16), 255, np.uint8)
    dire = np.broadcast_to(_checker(), (n, 3, 16, 16)).copy()
    return qt, bt, dire


SEEDS = {"valid_cf1": 1101, "valid_cf2": 1102, "noisy": 1103, "wrap": 1104, "ties": 1105, "qtdeep": 1106}
WRAP_POOL = 300


def label_sets():
    """(name, cf, (qt, bt, dire)) of every label case g11 holds the reference's answer for."""
    yield "valid_cf1", 1, valid_blocks(150, SEEDS["valid_cf1"], 1)
    yield "valid_cf2", 2, valid_blocks(150, SEEDS["valid_cf2"], 2)
    yield "noisy", 1, noisy_blocks(120, SEEDS["noisy"])
    yield "ties", 1, tie_blocks(40, SEEDS["ties"])
    yield "ties_cf2", 2, tie_blocks(40, SEEDS["ties"] + 1)
    yield "qtdeep", 1, qt_deep_blocks(20, SEEDS["qtdeep"])
    yield "bigtree_cf1", 1, big_tree_blocks()
    yield "bigtree_cf2", 2, big_tree_blocks()
    yield "overbudget", 1, over_budget_blocks()
    yield "wrap", 1, noisy_blocks(WRAP_POOL, SEEDS["wrap"], frac=0.05)   # g11 stores which of them change with int16 labels


# ------------------------------------------------------------------------------------------------ numpy restatement
def _split(x, y, h, w, mode):
    if mode == 0:
        return [(x, y, h, w)]
    if mode == 1:
        return [(x, y, h // 2, w), (x + h // 2, y, h // 2, w)]
    if mode == 2:
        return [(x, y, h, w // 2), (x, y + w // 2, h, w // 2)]
    if mode == 3:
        return [(x, y, h // 4, w), (x + h // 4, y, h // 2, w), (x + (h * 3) // 4, y, h // 4, w)]
    return [(x, y, h, w // 4), (x, y + w // 4, h, w // 2), (x, y + (w * 3) // 4, h, w // 4)]


def _can_split(bt, dire, cf, x, y, h, w, cur, depth):
    """can_split_mode_list (GenMSBtMap.py:123-186) on integers."""
    b = bt[x:x + h, y:y + w].astype(np.int16)
    if np.count_nonzero(b == cur[x:x + h, y:y + w]) >= L1 * h * w:
        return [0]
    d = dire[depth, x:x + h, y:y + w]
    hor, ver = int(np.count_nonzero(d == 1)), int(np.count_nonzero(d == -1))
    direction = 0
    if ver + hor >= L2 * h * w:
        if hor >= L3 * ver:
            direction = 1
        elif ver >= L3 * hor:
            direction = 2
    else:
        return [0]
    out = []
    for mode in (1, 2, 3, 4):
        ext = h if mode in (1, 3) else w
        div = (2 if mode <= 2 else 4) * cf
        if ext // div == 0 or ext % div != 0:
            continue
        if mode in (1, 3) and direction == 2 or mode in (2, 4) and direction == 1:
            continue
        ok = 0
        parts = _split(x, y, h, w, mode)
        for i, (sx, sy, sh, sw) in enumerate(parts):
            tgt = cur[sx:sx + sh, sy:sy + sw].astype(np.int16) + (2 if mode >= 3 and i != 1 else 1)
            sb = bt[sx:sx + sh, sy:sy + sw].astype(np.int16)
            minus, zero, npx = int(np.count_nonzero(sb < tgt)), int(np.count_nonzero(sb == tgt)), sh * sw
            if minus < npx * L4 and (zero < npx * L5 or zero > npx * (1 - L5)):
                ok += 1
        if ok == len(parts):
            out.append(mode)
    return out


class _Stop(Exception):
    pass


def region(bt, dire, cf, x, y, h, w, budget=BUDGET):
    """set_bt_sub_map (GenMSBtMap.py:326-364) for one QT region -> (maps u8[3][16][16] on the region, best leaf depth, leaves scored,
    over budget).  The leaf error wraps as the reference's u8 subtraction does; a best leaf at depth d < 3 gets the carry-down rule."""
    st = {"n": 0, "best": None}
    lb = bt[x:x + h, y:y + w].astype(np.int64)

    def leaf(maps):
        if st["n"] >= budget:
            raise _Stop
        st["n"] += 1
        d = len(maps) - 1
        err = int(lb.sum()) if d == 0 else int(((maps[d][x:x + h, y:y + w].astype(np.int64) - lb) % 256).sum())
        if st["best"] is None or err < st["best"][0]:
            st["best"] = (err, d, list(maps))

    def node(maps, cus):
        depth = len(maps) - 1
        if depth >= 3:
            leaf(maps)
            return
        lists = []
        for (cx, cy, ch, cw) in cus:
            lst = _can_split(bt, dire, cf, cx, cy, ch, cw, maps[-1], depth)
            if not lst:
                leaf(maps)
                return
            lists.append(lst)
        for combo in itertools.product(*lists):          # first CU slowest, as Search enumerates
            child = maps[-1].copy()
            ccus = []
            for (cx, cy, ch, cw), m in zip(cus, combo):
                parts = _split(cx, cy, ch, cw, m)
                ccus += parts
                if m:
                    for i, (sx, sy, sh, sw) in enumerate(parts):
                        child[sx:sx + sh, sy:sy + sw] += 2 if m >= 3 and i != 1 else 1
            node(maps + [child], ccus)

    stop = False
    try:
        node([np.zeros((16, 16), np.int16)], [(x, y, h, w)])
    except _Stop:
        stop = True
    err, d, maps = st["best"]
    out = np.zeros((3, 16, 16), np.uint8)
    if d > 0:
        for k in range(3):
            out[k] = maps[min(k + 1, d)]
    return out, d, st["n"], stop


def restate(qt, bt, dire, cf, budget=BUDGET, stats=None):
    """Map_to_SubMap(qt, bt, dire, cf).get_sub_map() with the library's status rules -> (msbt u8[3][16][16], status)."""
    msbt = np.zeros((3, 16, 16), np.uint8)
    status = 0

    def rec(depth, qx, qy):
        nonlocal status
        c = int(qt[qx, qy])
        sms = 8 >> depth
        if c == depth:
            x, y, s = 2 * qx, 2 * qy, 2 * sms
            maps, d, nleaf, stop = region(bt, dire, cf, x, y, s, s, budget)
            msbt[:, x:x + s, y:y + s] = maps[:, x:x + s, y:y + s]
            if d < 3:
                status |= INCONSISTENT
            if stop:
                status |= OVER_BUDGET
            if stats is not None:
                stats.append(nleaf)
        elif c > depth:
            if depth == 3:
                status |= QT_DEEP
                return
            for io in range(2):
                for jo in range(2):
                    rec(depth + 1, qx + io * sms // 2, qy + jo * sms // 2)

    rec(0, 0, 0)
    return msbt, status


def restate_batch(qt, bt, dire, cf, budget=BUDGET, stats=None):
    n = len(qt)
    out = np.zeros((n, 3, 16, 16), np.uint8)
    st = np.zeros(n, np.uint8)
    for i in range(n):
        out[i], st[i] = restate(qt[i], bt[i], dire[i], cf, budget, stats)
    return out, st


# ------------------------------------------------------------------------------------------------ DecLib-format dumps
SPLIT_CODE = {1: 2, 2: 3, 3: 4, 4: 5}   # mode (1 BT-H, 2 BT-V, 3 TT-H, 4 TT-V) -> PartSplit (UnitPartitioner.h: 2..5)
DONT_SPLIT, QUAD_SPLIT = 2000, 1


def _ctu_cus(rng, x0, y0, p_qt=0.5, p_mtt=0.55):
    """Leaf CUs of one 128x128 CTU in luma samples, in decoding order: (x, y, h, w, qtDepth, btDepth, mtDepth, codes[8]) with x the
    column.  The CTU is always QT-split once (qtDepth >= 1, VTM's implicit 128 -> 64 split), then QT to depth 1..4, then up to three
    MTT layers down to 4-sample sides."""
    out = []

    def mtt(x, y, h, w, qd, bd, md, codes):
        legal = []
        if md < 3:
            if h >= 8: legal.append(1)
            if w >= 8: legal.append(2)
            if h >= 16: legal.append(3)
            if w >= 16: legal.append(4)
        if not legal or rng.random() > p_mtt:
            out.append((x, y, h, w, qd, bd, md, codes + [DONT_SPLIT] * (8 - len(codes))))
            return
        mode = legal[rng.integers(len(legal))]
        for (sr, sc, sh, sw, inc) in synth._split(y, x, h, w, mode):      # synth works in (row, col)
            mtt(sc, sr, sh, sw, qd, bd + inc, md + 1, codes + [SPLIT_CODE[mode]])

    def quad(x, y, s, qd):
        if qd == 0 or (qd < 3 and rng.random() < p_qt) or (qd == 3 and rng.random() < p_qt * 0.4):
            h = s // 2
            for (dx, dy) in ((0, 0), (h, 0), (0, h), (h, h)):
                quad(x + dx, y + dy, h, qd + 1)
        else:
            mtt(x, y, s, s, qd, 0, 0, [QUAD_SPLIT] * qd)

    quad(x0, y0, 128, 0)
    return out


def make_dump(seed, frames_written, height, width, chroma, unknown_rate=0.0):
    """Text of a Save_Depth_fal dump (DecLib.cpp:1011-1047): "frame++", then per CU 'x y h w depth qt bt mt s0 .. s7 ' and a newline."""
    rng = np.random.default_rng(seed)
    lines = []
    for _ in range(frames_written):
        lines.append("frame++\n")
        for cy in range(0, height, 128):
            for cx in range(0, width, 128):
                for (x, y, h, w, qd, bd, md, codes) in _ctu_cus(rng, cx, cy):
                    codes = list(codes)
                    if unknown_rate and rng.random() < unknown_rate:
                        codes[qd + int(rng.integers(0, 3))] = int(rng.choice([0, 1, 6, 7, 1999]))
                    if chroma:
                        x, y, h, w = x // 2, y // 2, h // 2, w // 2
                    vals = [x, y, h, w, 2 * qd + bd, qd, bd, md] + codes
                    lines.append(" ".join(str(v) for v in vals) + " \n")
    return "".join(lines)


# (name, seed, frames written, frames, height, width, chroma, unknown-code rate)
DUMPS = (
    ("luma", 2101, 2, 2, 192, 256, False, 0.0),
    ("chroma", 2102, 2, 2, 192, 256, True, 0.0),
    ("short_odd", 2103, 1, 3, 240, 416, False, 0.03),     # fewer frames than `frames`; 416x240 is not a multiple of 64
    ("chroma_unknown", 2104, 2, 2, 240, 416, True, 0.05),
)

# gen_labels on a synthesized dump directory: two sequences, both components, two QPs
PIPE_SEQS = (("SeqA", 256, 128, 9), ("SeqB", 192, 192, 4))   # name, width, height, frames (ssRatio 8: 2 and 1 dumped frames)
PIPE_QPS = (22, 37)
PIPE_SS = 8


def write_pipe_dir(d):
    """The dump directory and sequence table of the pipeline case; returns the table's path.  SeqA's dumps carry CreateDataSet's
    names, SeqB's DecLib's."""
    os.makedirs(d, exist_ok=True)
    for si, (name, w, h, f) in enumerate(PIPE_SEQS):
        sub = (f + PIPE_SS - 1) // PIPE_SS
        for ci, comp in enumerate(("Luma", "Chroma")):
            for qp in PIPE_QPS:
                suffix = "_Partition.txt" if si == 0 else "_Partition_FastOff_LFNST0.txt"
                with open(os.path.join(d, "%s_QP%d_%s%s" % (name, qp, comp, suffix)), "w") as fp:
                    fp.write(make_dump(3000 + 97 * si + 13 * ci + qp, sub, h, w, comp == "Chroma"))
    table = os.path.join(d, "seqs.txt")
    with open(table, "w") as fp:
        for (name, w, h, f) in PIPE_SEQS:
            fp.write("%s,%s.yuv,%d,%d,%d,30\n" % (name, name, w, h, f))
    return table
