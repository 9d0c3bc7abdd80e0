"""CPU: the parity yardstick (oracle/parity.py) on hand-made arrays of two to four blocks - the extreme blocks against their literal
construction, each of the three rounding boundaries of the audit at its margin, the uint8 cast of the oracle's QT map, the per-block
maximum, the tolerance of the synthetic extremes and the nine tensors of the range-stress weights."""
import numpy as np

from oracle import parity as Y

MARGIN = 2.0 ** -10        # a power of two: .5 +- MARGIN and .5 +- 2 MARGIN are exact in float32 near 1


def _blocks(n, seed=5):
    rng = np.random.default_rng(seed)
    return (rng.integers(0, 256, (n, 68, 68), dtype=np.uint8), rng.integers(0, 256, (n, 34, 34), dtype=np.uint8),
            rng.integers(0, 256, (n, 34, 34), dtype=np.uint8))


def test_extreme_blocks_are_the_literal_construction():
    y, u, v = _blocks(6)
    y0, u0, v0 = y.copy(), u.copy(), v.copy()
    Y.extreme_blocks(y, u, v, 37)
    rng = np.random.default_rng(37)
    assert not y[0].any() and not u[0].any() and not v[0].any()
    assert (y[1] == 255).all() and (u[1] == 255).all() and (v[1] == 255).all()
    for a in (y, u, v):
        assert np.array_equal(a[2], rng.integers(0, 256, a[2].shape))
    board = np.array([[255 if (i // 2 + j // 2) % 2 else 0 for j in range(68)] for i in range(68)], np.uint8)
    assert np.array_equal(y[3], board) and np.array_equal(u[3], u0[3]) and np.array_equal(v[3], v0[3])
    assert np.array_equal(y[4:], y0[4:]) and np.array_equal(u[4:], u0[4:]) and np.array_equal(v[4:], v0[4:])
    y2, u2, v2 = y0.copy(), u0.copy(), v0.copy()
    Y.extreme_blocks(y2, u2, v2, count=2)                   # the flat pair alone
    assert np.array_equal(y2[:2], y[:2]) and np.array_equal(u2[:2], u[:2]) and np.array_equal(y2[2:], y0[2:]) and np.array_equal(v2[2:], v0[2:])


def _quiet(n):
    """Oracle logits of n blocks far from every boundary, and flags that agree with themselves."""
    oq = np.full((n, 1, 8, 8), 1.25, np.float32)
    obt = np.full((n, 3, 16, 16), 2.25, np.float32)
    od = np.full((n, 3, 16, 16), 0.875, np.float32)
    flags = (np.zeros((n, 16, 16), np.uint8), np.zeros((n, 16, 16), np.uint8), np.ones((n, 8, 8), np.float32), np.zeros((n, 3, 16, 16), np.int8))
    return oq, obt, od, flags


def _device(flags):
    return flags[0].copy(), flags[1].copy(), flags[2].astype(np.uint8), flags[3].copy()


def test_boundary_audit_each_boundary_at_its_margin():
    """Block 0: a value just inside the margin of the boundary, block 1: exactly at the margin (the test is strict), block 2: just
    outside, block 3: quiet.  For the pooled QT map, np.round of the depth, and the +-.5 thresholds of the direction on both signs."""
    inside, at, outside = 0.5 + MARGIN / 2, 0.5 + MARGIN, 0.5 + 2 * MARGIN
    for which in ("qt", "qt_below", "bt", "bt_below", "dire", "dire_negative"):
        oq, obt, od, flags = _quiet(4)
        for blk, frac in enumerate((inside, at, outside)):
            if which == "qt":
                oq[blk, 0, 3, 4] = 1.0 + frac             # the largest of its 2x2 cell: the pooled value
            elif which == "qt_below":
                oq[blk, 0, 2:4, 4:6] = 2.0 - frac         # the whole cell: the pool takes its maximum
            elif which == "bt":
                obt[blk, 2, 5, 7] = 3.0 + frac
            elif which == "bt_below":
                obt[blk, 0, 0, 15] = -1.0 - frac          # x - floor(x) = 1 - frac
            elif which == "dire":
                od[blk, 1, 9, 0] = frac
            else:
                od[blk, 0, 15, 15] = -frac
        bad, risky = Y.boundary_audit(oq, obt, od, _device(flags), flags, MARGIN)
        assert risky.tolist() == [True, False, False, False], which
        assert not bad.any(), which


def test_boundary_audit_pools_the_qt_map():
    """A QT value near a boundary that is NOT the maximum of its 2x2 cell is not a risk: Metrics.py:632 pools first."""
    oq, obt, od, flags = _quiet(2)
    oq[0, 0, 2:4, 4:6] = 2.25
    oq[0, 0, 3, 4] = 1.5
    _, risky = Y.boundary_audit(oq, obt, od, _device(flags), flags, MARGIN)
    assert not risky.any()


def test_boundary_audit_a_mismatch_in_a_quiet_block_is_bad_and_not_risky():
    for k, cell in enumerate(((1, 0, 0), (2, 15, 15), (0, 7, 7), (3, 2, 8, 8))):
        oq, obt, od, flags = _quiet(4)
        obt[3, 0, 0, 0] = 1.5                              # block 3 is risky
        got = list(_device(flags))
        got[k][cell] += 1                                  # one flag of array k differs in block cell[0]
        bad, risky = Y.boundary_audit(oq, obt, od, got, flags, MARGIN)
        assert risky.tolist() == [False, False, False, True]
        assert np.flatnonzero(bad).tolist() == [cell[0]], k
        assert (bad & ~risky).tolist() == [b == cell[0] and b != 3 for b in range(4)], k


def test_flags_equal_casts_the_oracles_qt_map():
    _, _, _, flags = _quiet(2)
    flags[2][1, 3, 3] = 3.0
    got = _device(flags)
    assert got[2].dtype == np.uint8 and flags[2].dtype == np.float32
    assert Y.flags_equal(got, flags) and not Y.blocks_differing(got, flags).any()
    for k in range(4):
        off = [a.copy() for a in got]
        off[k][(1,) + (0,) * (off[k].ndim - 1)] += 1
        assert not Y.flags_equal(off, flags), k
        assert Y.blocks_differing(off, flags).tolist() == [False, True], k
    flags[2][0, 0, 0] = np.nan                             # a NaN the reference keeps: 0 on the device
    got[2][0, 0, 0] = 0
    assert Y.flags_equal(got, flags, nan_to_zero=True) and not Y.blocks_differing(got, flags, nan_to_zero=True).any()
    got[2][0, 0, 0] = 1
    assert not Y.flags_equal(got, flags, nan_to_zero=True) and Y.blocks_differing(got, flags, nan_to_zero=True).tolist() == [True, False]


def test_per_block_error_picks_the_block_and_the_array():
    oq, obt, od, _ = _quiet(3)
    qt, bt, dire = oq.copy(), obt.copy(), od.copy()
    qt[0, 0, 7, 7] += 0.25
    bt[1, 2, 0, 0] -= 0.5
    dire[1, 0, 3, 3] += 0.125
    err = Y.per_block_error((qt, bt, dire), (oq, obt, od))
    assert err.dtype == np.float32 and err.tolist() == [0.25, 0.5, 0.0]
    literal = np.maximum(np.abs(qt - oq).reshape(3, -1).max(1), np.maximum(np.abs(bt - obt).reshape(3, -1).max(1), np.abs(dire - od).reshape(3, -1).max(1)))
    assert np.array_equal(err, literal)
    assert Y.per_block_max((oq, obt, od)).tolist() == [2.25, 2.25, 2.25]


def test_block_tolerance_is_relative_only_for_the_extremes_beyond_the_range():
    mag = np.array([4.0, 8.0, 300.0, 16.0, 300.0, 2.0])
    assert Y.block_tolerance(1e-3, mag).tolist() == [1e-3, 1e-3, 1e-3 * 37.5, 2e-3, 1e-3, 1e-3]
    assert Y.block_tolerance(1e-3, mag, n_extremes=0).tolist() == [1e-3] * 6


def test_range_stress_weights_change_exactly_the_tensors_their_docstring_names():
    """The three stems' weights and biases (x K) and the first convolution and shortcut of B1.0, B2.0, B3.0 (/ K): twelve tensors."""
    from pmp_vvc_tip2023_amd import synth
    base = synth.synth_msbd_weights("Luma", 22)
    same = Y.range_stress_weights(1.0)
    assert list(same) == list(base)
    assert all(same[k].dtype == base[k].dtype and np.array_equal(same[k].view(np.uint32), base[k].view(np.uint32)) for k in base)
    w = Y.range_stress_weights(2.0 ** 17)
    changed = sorted(k for k in base if not np.array_equal(w[k], base[k]))
    stems = ["conv_b1_%d.%s" % (i, p) for i in (1, 2, 3) for p in ("bias", "weight")]
    firsts = ["trunk_B%d.0.%s.0.weight" % (i, p) for i in (1, 2, 3) for p in ("left", "shortcut")]
    assert changed == sorted(stems + firsts) and list(w) == list(base)
    assert all(np.array_equal(w[k], base[k] * np.float32(2.0 ** 17)) for k in stems)
    assert all(np.array_equal(w[k] * np.float32(2.0 ** 17), base[k]) for k in firsts)
