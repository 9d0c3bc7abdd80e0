"""CPU: guard_cases' restatement of the divergence guard's census and record rule (include/pmp.h, TRAINING STEP), which
test_gpu_grad_guard.py holds the kernels to bit for bit.

The census against the correctly rounded sum: math.fsum of the exact squares (a float32 squared is exact in float64).  The header's
order is 16 sequential additions, an 8-level tree, and the same again over the tiles' partials: at most 48 roundings of relative
size 2^-53 on sums of non-negative terms, 5.4e-15 in the worst case and far less on sums that a few large squares dominate; the bound
asked of every case is a relative distance of 1e-15.  The count against ~np.isfinite.  The record rule at its edges."""
import math

import numpy as np
import pytest

import guard_cases as G


@pytest.mark.parametrize("name,plant", G.CASES, ids=["%s-%s" % c for c in G.CASES])
def test_census_is_the_rounded_sum_of_the_finite_squares_and_the_count_of_the_rest(name, plant):
    ts = G.table(name, plant)
    sumsq, nonfinite, partials = G.census(ts)
    want = G.exact_sumsq(ts)
    assert want > 0 and math.isfinite(want)
    assert abs(sumsq - want) <= 1e-15 * want, (sumsq, want, abs(sumsq - want) / want)
    assert nonfinite == sum(int((~np.isfinite(t)).sum()) for t in ts) == len(G.PLANTS[plant])
    assert len(partials) == sum(-(-n // G.TILE) for n in G.TABLES[name]) and np.isfinite(partials).all()


def test_float32_accumulation_would_visibly_differ():
    ts = G.table("nine")
    sumsq = G.census(ts)[0]
    with np.errstate(over="ignore"):
        f32 = float(sum(np.sum(t * t, dtype=np.float32) for t in ts))
    assert not abs(f32 - sumsq) <= 1e-9 * sumsq


def _by_the_letter(values):
    """The header's text for one round, lane by lane in plain Python floats: values[i] belongs to lane i % 256"""
    a = [0.0] * 256
    for l in range(256):
        for i in range(l, len(values), 256):
            a[l] = a[l] + values[i]
    h = 128
    while h >= 1:
        for l in range(h):
            a[l] = a[l] + a[l + h]
        h //= 2
    return a[0]


def test_the_order_is_the_headers():
    """The vectorised restatement against the header's text taken by the letter, on two tensors of three tiles whose sum depends on
    the order (a plain left-to-right sum gives other bits)"""
    ts = [t for t in G.table("nine") if t.size in (4097, 2 * 4096 + 1)][:2]
    ts = [ts[0][:4097], ts[1][:4100]]
    sq = lambda t: [float(v) * float(v) for v in t]
    partials = [_by_the_letter(sq(t[b:b + 4096])) for t in ts for b in range(0, t.size, 4096)]
    sumsq, _, got = G.census(ts)
    assert len(partials) == 4 and got.tolist() == partials and sumsq == _by_the_letter(partials)
    rng = np.random.default_rng(3)
    t = rng.uniform(0.5, 1.5, 4096).astype(np.float32)
    left_to_right = 0.0
    for v in sq(t):
        left_to_right += v
    assert G.census([t])[0] == _by_the_letter(sq(t)) != left_to_right


def test_record_rule_at_its_edges():
    r = G.record(1.0, 0, max_norm=1.0)                    # norm == max_norm: 1 / (1 + 1e-6) < 1, as clip_grad_norm_ scales
    assert r["norm"] == 1.0 and r["coef"] == np.float32(1.0 / (1.0 + 1e-6)) < 1 and r["action"] == G.ACTION_CLIP
    r = G.record(0.0, 0, max_norm=1.0)                    # norm 0: c = 1e6, no clipping
    assert r["norm"] == 0.0 and r["coef"] == 1.0 and r["action"] == 0
    r = G.record(1e30, 0, max_norm=0.0)                   # max_norm 0: off
    assert r["coef"] == 1.0 and r["action"] == 0 and r["norm"] == 1e15
    r = G.record(4.0, 3, max_norm=0.0, skip_nonfinite=False)   # a NaN, and nobody asked to skip
    assert r["nonfinite"] == 3 and r["action"] == 0 and r["coef"] == 1.0 and r["norm"] == 2.0
    r = G.record(4.0, 3, max_norm=1.0, skip_nonfinite=True)
    assert r["action"] == G.ACTION_SKIP | G.ACTION_CLIP and r["coef"] == np.float32(1.0 / (2.0 + 1e-6))
    r = G.record(1e18, 0, max_norm=1e9)                   # c = 1 - 1e-15 in double, 1.0 as a float: no multiply, no clip bit
    assert r["norm"] == 1e9 and 1e9 / (1e9 + 1e-6) < 1 and r["coef"] == 1.0 and r["action"] == 0
    assert isinstance(r["coef"], np.float32)


def test_counters_follow_a_scripted_sequence():
    take, clip, skip = {"action": 0, "norm": 1.0}, {"action": 2, "norm": 3.0}, {"action": 1, "norm": 2.0}
    both = {"action": 3, "norm": 9.0}
    s = G.counters([take, skip, skip, clip, skip, both, skip, skip, take])
    assert s == {"steps": 9, "skipped": 6, "clipped": 1, "run": 0, "max_run": 4, "max_norm": 9.0}     # a skipped step is not a clipped one
    assert G.counters([skip], s)["run"] == 1 and G.counters([skip], s)["max_run"] == 4
