"""A numpy restatement of GenMSBtMap.Map_to_SubMap.get_partition / map_to_parititon (GenMSBtMap.py:262-312, :377-382) - the split flags of
the labels' own partition (include/pmp.h: pmp_label_partition) - and of the file get_sequence_partition_for_VTM writes (:384-432).

Built on tests/msbt_cases.py: its label sets, its can_split_mode_list and split rules, and its leaf budget.  msbt_cases.region keeps the
best leaf's MAPS; the painting needs the best leaf's CU LIST, so region_cus below walks the same tree in the same order and keeps that
(test_label_partition_cpu.py checks that both walks agree on depth, leaf count, budget stop and leaf map).  The restatement defines the
result where the library deviates from the reference by rule: the over-budget block.  Not a test module: no test_ prefix."""
import itertools
import os

import numpy as np

import msbt_cases as K

GOLDEN = os.path.join(K.ROOT, "tests", "golden", "g13_label_partition.npz")
QT_DEEP, OVER_BUDGET = K.QT_DEEP, K.OVER_BUDGET


def label_sets():
    """(name, cf, (qt, bt, dire)) of every case g13 holds the reference's answer for: msbt_cases' sets without the wrap pool."""
    for name, cf, x in K.label_sets():
        if name != "wrap":
            yield name, cf, x


def region_cus(bt, dire, cf, x, y, h, w, budget=K.BUDGET):
    """set_bt_partition_vector's search (:262-278) for one QT region -> (CU list of the best leaf, its depth, its map, leaves scored,
    over budget).  Leaf error with the reference's u8 wrap, first minimum in DFS leaf order, msbt_cases' budget rule."""
    st = {"n": 0, "best": None}
    lb = bt[x:x + h, y:y + w].astype(np.int64)

    def leaf(maps, cus):
        if st["n"] >= budget:
            raise K._Stop
        st["n"] += 1
        d = len(maps) - 1
        err = int(lb.sum()) if d == 0 else int(((maps[d][x:x + h, y:y + w].astype(np.int64) - lb) % 256).sum())
        if st["best"] is None or err < st["best"][0]:
            st["best"] = (err, d, maps[d].copy(), list(cus))

    def node(maps, cus):
        depth = len(maps) - 1
        if depth >= 3:
            leaf(maps, cus)
            return
        lists = []
        for (cx, cy, ch, cw) in cus:
            lst = K._can_split(bt, dire, cf, cx, cy, ch, cw, maps[-1], depth)
            if not lst:
                leaf(maps, cus)
                return
            lists.append(lst)
        for combo in itertools.product(*lists):          # first CU slowest, as Search enumerates
            child = maps[-1].copy()
            ccus = []
            for (cx, cy, ch, cw), m in zip(cus, combo):
                parts = K._split(cx, cy, ch, cw, m)
                ccus += parts
                if m:
                    for i, (sx, sy, sh, sw) in enumerate(parts):
                        child[sx:sx + sh, sy:sy + sw] += 2 if m >= 3 and i != 1 else 1
            node(maps + [child], ccus)

    stop = False
    try:
        node([np.zeros((16, 16), np.int16)], [(x, y, h, w)])
    except K._Stop:
        stop = True
    _, d, m, cus = st["best"]
    return cus, d, m, st["n"], stop


def restate(qt, bt, dire, cf, budget=K.BUDGET):
    """map_to_parititon(qt, bt, dire, cf) with the library's status rules -> (hor u8[16][16], ver u8[16][16], status)."""
    vec = np.zeros((2, 17, 17), np.uint8)                 # par_vec (:99); row and column 16 are cropped away (:382)
    status = 0

    def rec(depth, qx, qy):
        nonlocal status
        c = int(qt[qx, qy])
        sms = 8 >> depth
        if c == depth:
            cus, _, _, _, stop = region_cus(bt, dire, cf, 2 * qx, 2 * qy, 2 * sms, 2 * sms, budget)
            if stop:
                status |= OVER_BUDGET
            for (x, y, h, w) in cus:                      # :285-292
                vec[0, x, y:y + w] = 1
                vec[0, x + h, y:y + w] = 1
                vec[1, x:x + h, y] = 1
                vec[1, x:x + h, y + w] = 1
        elif c > depth:
            vec[0, 2 * qx + sms, 2 * qy:2 * qy + 2 * sms] = 1     # :300-304
            vec[1, 2 * qx:2 * qx + 2 * sms, 2 * qy + sms] = 1
            if depth == 3:                                # the reference recurses on empty regions from here: nothing more is painted
                status |= QT_DEEP
                return
            for io in range(2):
                for jo in range(2):
                    rec(depth + 1, qx + io * sms // 2, qy + jo * sms // 2)

    rec(0, 0, 0)
    return vec[0, :16, :16].copy(), vec[1, :16, :16].copy(), status


def restate_batch(qt, bt, dire, cf, budget=K.BUDGET):
    n = len(qt)
    hor = np.zeros((n, 16, 16), np.uint8); ver = np.zeros((n, 16, 16), np.uint8); st = np.zeros(n, np.uint8)
    for i in range(n):
        hor[i], ver[i], st[i] = restate(qt[i], bt[i], dire[i], cf, budget)
    return hor, ver, st


_ALL = {}


def restated_sets():
    """{name: (cf, (qt, bt, dire), hor, ver, status)} for every set of label_sets(), computed once per process and shared."""
    if not _ALL:
        for name, cf, x in label_sets():
            _ALL[name] = (cf, x) + restate_batch(*x, cf)
    return _ALL


# ------------------------------------------------------------------------------------------------ the file of the pipe sequences
def pipe_cases():
    """(seq, comp, qp, width, height, dumped frames) of every file get_sequence_partition_for_VTM writes for msbt_cases.write_pipe_dir."""
    for (name, w, h, f) in K.PIPE_SEQS:
        for comp in ("Luma", "Chroma"):
            for qp in K.PIPE_QPS:
                yield name, comp, qp, w, h, (f + K.PIPE_SS - 1) // K.PIPE_SS


def pipe_key(seq, comp, qp):
    return "file_%s_%s_%d_" % (seq, comp, qp)


def pipe_dump_path(d, seq, comp, qp):
    for suf in ("_Partition.txt", "_Partition_FastOff_LFNST0.txt"):
        p = os.path.join(d, "%s_QP%d_%s%s" % (seq, qp, comp, suf))
        if os.path.isfile(p):
            return p
    raise FileNotFoundError((seq, comp, qp))


def map_255_to_minus1(text, frames, height, width):
    """The reference's text with the '255' lines of its direction sections (dire cast to u8, :413) rewritten as '-1'; also returns how
    many lines changed.  Lines outside the direction sections are left alone."""
    lines = text.split("\n")
    assert lines[-1] == ""
    lines = lines[:-1]
    cells = 256 * (height // 64) * (width // 64)
    per = 5 * cells + cells // 4
    assert len(lines) == frames * per
    changed = 0
    for f in range(frames):
        lo = f * per + 2 * cells + cells // 4
        for i in range(lo, (f + 1) * per):
            if lines[i] == "255":
                lines[i] = "-1"
                changed += 1
    return "\n".join(lines) + "\n", changed
