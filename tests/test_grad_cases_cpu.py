"""CPU: the table of tests/grad_cases.py - what tests/test_gpu_grad_sweep.py runs on the GPU - is what it claims to be.  Every exact
case stays inside float32's exact integers in any order of summation; the table reaches every instantiation of the training kernels
(held against the kernel symbols of the built library), every map, partition edge and value kind; the constant of the weight
gradients' bound is twice what an emulation of the kernels' order of summation reaches; the restatement equals the reference's numbers
on the new ground (tests/golden/g17_grad_sweep.npz, tools/gen_golden_grad_sweep.py)."""
import functools
import os
import re

import numpy as np
import pytest
import torch

from conftest import golden
import grad_cases as G
import resblock_cases as K
import trunk_cases as T
from cases_common import LIB, kernel_symbols


@functools.lru_cache(maxsize=None)
def block(name):
    """-> (case, float64 restatement); computed once, never changed."""
    c = G.make_block(name)
    return c, K.restate(c)


@functools.lru_cache(maxsize=None)
def float_case(name):
    """-> (case, float_reference(case)); computed once, never changed."""
    c = G.make_block(*G.FLOAT[name])
    return c, G.float_reference(c)


# ---- 1. the exact cases are exact
@pytest.mark.parametrize("name", list(G.BLOCKS))
def test_exact_block_case_fits_float32_in_any_order(name):
    c, r = block(name)
    n, h, w, cin, cout, k = c["shape"]
    assert c["x"].shape == (n, cin, h, w) and c["w0"].shape == (cout, cin, k, k) and (c["wsc"] is None) == (cin == cout)
    assert K.worst_partial_sum(c) < 2 ** 24
    r32 = K.restate(c, torch.float32)
    for key in K.OUTPUTS:
        if r[key] is None:
            assert r32[key] is None
            continue
        assert r32[key].dtype == np.float32 and np.array_equal(r32[key].astype(np.float64), r[key]), (name, key, "float32 is not exact")
    for key in ("t", "out"):                          # the `> 0` rule of the masks has both sides and the edge
        assert 0.3 <= float((r[key] > 0).mean()) <= 0.7 and (r[key] == 0).any(), (name, key)


@pytest.mark.parametrize("name", list(G.TRUNKS))
def test_exact_trunk_case_fits_float32_in_any_order(name):
    c, r = G.trunk_exact(name)
    assert T.worst_partial_sum(c) < (2 ** 23 if name == G.SUBNORMAL_TRUNK else 2 ** 24)
    r32 = T.flat(T.restate(c, torch.float32))
    assert sorted(r32) == sorted(r)
    for key, v in r.items():
        assert r32[key].dtype == np.float32 and np.array_equal(r32[key].astype(np.float64), v), (name, key, "float32 is not exact")
    # The positive share of t and out.  The sparse +-1 weights leave single tensors of the narrow blocks outside 0.3 .. 0.7 (a 1-channel
    # t of three non-zero taps is positive at 4 % of its pixels, a 15 -> 17 block's out at 75 %), so a tensor is held to 0.03 .. 0.8
    # and the case as a whole, the mean over its t_i and out_i, to the 0.3 .. 0.7 the block cases meet tensor by tensor.
    shares = []
    for key, v in r.items():
        if key[0] in "to":                            # t<i>, out<i>
            assert (v == 0).any() and (v == np.rint(v)).all(), (name, key)
            shares.append(float((v > 0).mean()))
            assert 0.03 <= shares[-1] <= 0.8, (name, key, shares[-1])
    assert 0.3 <= float(np.mean(shares)) <= 0.7, (name, shares)


def test_trunk_table_is_what_the_sweep_promises():
    shapes = list(G.TRUNKS.values())
    assert 13 <= len(shapes) <= 16
    assert {len(s[4]) for s in shapes} == set(range(1, 9))
    assert sum(len(s[4]) == 8 for s in shapes) >= 2 and any(len(s[4]) == 8 and s[5] for s in shapes)
    assert sum(any(k == 5 for _, k in s[4][1:]) for s in shapes) >= 3                   # k = 5 behind the first block
    ragged = {c for v in G.RAGGED.values() for c in v}
    assert all(c in ragged | {16} for s in shapes for c in [s[3]] + [co for co, _ in s[4]])
    assert {c for s in shapes for c in [s[3]] + [co for co, _ in s[4]]} >= ragged
    steps = [(G.pad(ci), G.pad(co)) for s in shapes for ci, co, _ in T.block_shapes(s)]
    assert any(a < b for a, b in steps) and any(a > b for a, b in steps)                # widening and narrowing
    assert any(s[5] and 33 <= s[4][-1][0] <= 63 for s in shapes)                        # a pool behind a 64-padded ragged block
    assert {(s[1], s[2]) for s in shapes} == {(16, 16), (32, 16), (16, 32), (48, 32), (16, 256)}
    assert {s[0] for s in shapes} == {1, 2, 3}
    assert sum(T.tied_positive_windows(G.trunk_exact(nm)[1]["out%d" % (len(s[4]) - 1)]) for nm, s in G.TRUNKS.items() if s[5]) >= 10
    for nm in G.TRUNK_FLOAT:
        assert nm in G.TRUNKS
    assert any(len(G.TRUNKS[nm][4]) == 8 for nm in G.TRUNK_FLOAT)
    assert any(any(k == 5 for _, k in G.TRUNKS[nm][4][1:]) for nm in G.TRUNK_FLOAT)
    s = G.TRUNKS[G.SUBNORMAL_TRUNK]
    assert s[5] == 1 and len(s[4]) <= 3


def test_subnormal_trunk_is_the_base_case_scaled():
    """Float64 on the scaled x gives the scaled restatement, and every scaled value is an exact float32 subnormal."""
    c, r = G.trunk_exact(G.SUBNORMAL_TRUNK)
    sc = G.scaled_trunk(c)
    assert np.array_equal(sc["x"].astype(np.float64), c["x"].astype(np.float64) * G.SUB)
    want, got = G.scaled_restatement(r), T.flat(T.restate(sc))
    for key, v in want.items():
        assert np.array_equal(got[key], v), key
        assert np.array_equal(K.as_f32(v).astype(np.float64), v), (key, "not a float32 value")
        if key != "g_x":
            assert np.abs(v).max() < 2.0 ** -126 and np.abs(v).max() > 0, key
            assert np.array_equal(v > 0, r[key] > 0), (key, "a mask changed")


# ---- 2. the table's reach
def test_every_block_case_is_in_a_gpu_group():
    groups = [list(G.BLOCKS)[g::G.NGROUPS] for g in range(G.NGROUPS)]
    assert all(groups) and sorted(nm for names in groups for nm in names) == sorted(G.BLOCKS)


def test_block_table_reaches_every_instantiation_and_edge():
    shapes = G.BLOCKS
    assert len(G.GRID) == 36 and len(shapes) == len(G.GRID) + len(G.EDGES) and set(G.FLOAT.values()) <= {(nm, kd) for nm in shapes for kd in G.KINDS}
    triples = {(k, nco, cb) for s in shapes.values() for _, k, nco, cb, _, _ in G.wgrads(s)}
    assert triples == {(k, nco, cb) for k in (1, 3, 5) for nco in (1, 2, 4) for cb in (1, 2, 4)}
    # the data gradient's packing: every (k, pad(cin), pad(cout)), both with the pads' counts and with ragged ones
    for tag in ("p_", "r_"):
        cells = {(s[5], G.pad(s[3]), G.pad(s[4])) for nm, s in G.GRID.items() if nm.startswith(tag)}
        assert cells == {(k, a, b) for k in (3, 5) for a in G.PADS for b in G.PADS}, tag
    assert all(s[3] != s[4] for nm, s in G.GRID.items() if nm.startswith("r_"))
    assert all(s[3] == G.pad(s[3]) and s[4] == G.pad(s[4]) for nm, s in G.GRID.items() if nm.startswith("p_"))
    assert {c for nm, s in G.GRID.items() if nm.startswith("r_") for c in s[3:5]} == {c for v in G.RAGGED.values() for c in v}
    assert {(s[1], s[2]) for s in G.GRID.values()} == set(G.MAPS) and any(s[1] > s[2] for s in shapes.values())
    assert {s[0] for s in G.GRID.values()} == set(G.NS) and {1, 256} <= {s[0] for s in shapes.values()}
    assert any(s[1] == 256 and s[2] == 256 for s in shapes.values())
    # the partition of the reduction: 1, 2, 3 items; below, at and above 2 * cap for every Ca; an uneven tail behind the cap
    parts = {(cb * 16, items) for s in shapes.values() for out, k, nco, cb, items, np_ in G.wgrads(s) if out != "g_w2"}
    parts |= {(nco * 16, items) for s in shapes.values() for out, k, nco, cb, items, np_ in G.wgrads(s) if out == "g_w2"}
    assert {items for _, items in parts} >= {1, 2, 3}
    for ca in G.PADS:
        cap2 = 2 * 256 // (ca // 16)
        mine = sorted(items for a, items in parts if a == ca and cap2 - 2 <= items <= cap2 + 2)
        assert mine[0] < cap2 and cap2 in mine and mine[-1] > cap2, (ca, mine)
        assert G.wgrad_np(1, 16, 16 * mine[-1], ca)[1] == cap2 // 2                  # (a shape only for the formula) NP stays at the cap
    assert all(k == 3 and cout <= 16 for _, _, _, _, cout, k in G.EDGES.values())
    # the float share: every kind, every (K, NCO) pair, chains of at most 2048 terms
    assert 20 <= len(G.FLOAT) <= 28 and {kd for _, kd in G.FLOAT.values()} == set(G.KINDS)
    pairs = {(k, nco) for nm, _ in G.FLOAT.values() for _, k, nco, _, _, _ in G.wgrads(shapes[nm])}
    assert pairs == {(k, nco) for k in (1, 3, 5) for nco in (1, 2, 4)}
    chains = [-(-items // np_) * 256 for nm, _ in G.FLOAT.values() for _, _, _, _, items, np_ in G.wgrads(shapes[nm])]
    assert max(chains) <= 2048 and max(chains) >= 768
    assert len(G.MASK_EDGES) == 2 and {s[5] for s in G.MASK_EDGES.values()} == {3, 5}


_PATTERN = re.compile(G.SYMBOL_PATTERN)


def test_training_kernel_table_matches_the_library_and_the_cases_reach_it():
    syms = kernel_symbols(LIB, _PATTERN)
    table = set(G.INSTANTIATIONS)
    assert len(table) == len(G.INSTANTIATIONS) == 18
    assert syms == table, "in the library, not in the table: %s; in the table, not in the library: %s" % (sorted(syms - table), sorted(table - syms))
    reached = set()
    for s in G.BLOCKS.values():
        reached |= G.block_kernels(s)
    assert reached == table - {"blocked_relu_kernel<1>", "grad_to_blocked_kernel<0>", "grad_to_blocked_kernel<1>", "pool_to_dense_kernel"}
    for s in G.TRUNKS.values():
        reached |= G.trunk_kernels(s)
    assert reached == table


def test_cases_tell_transposed_taps_and_a_mask_of_zero_apart():
    """What the bit-for-bit comparison can see: a weight gradient with dy and dx swapped differs on every k x (NCO) cell of the grid, and
    a ReLU mask that lets t == 0 through (`>= 0`) changes g_w0 of every trunk case."""
    for name, s in G.GRID.items():
        if name.startswith("p_") and s[1] * s[2] <= 32 * 32:
            r = block(name)[1]
            for key in ("g_w0", "g_w2"):
                assert not np.array_equal(r[key], r[key].transpose(0, 1, 3, 2)), (name, key)
    for name in G.TRUNKS:
        c = G.make_trunk(name)
        r = T.restate(c)
        changed = False
        for i, (w0, w2, wsc) in enumerate(c["blocks"]):
            t = np.where(r["t"][i] == 0, 1e-300, r["t"][i])                  # positive for the mask, nothing for the sums
            b = K.backward(c["x"] if i == 0 else r["out"][i - 1], t, r["out"][i], w0, w2, wsc, r["g_out"][i])
            changed = changed or not np.array_equal(np.rint(b["g_w0"]), r["g_w"][i][0])
        assert changed, name


# ---- 3. the float cases: the bound's constant comes from the emulated order of summation
@pytest.mark.parametrize("name", list(G.FLOAT))
def test_emulated_order_stays_within_half_the_bound(name):
    c, (t32, out32, ref, bnd, parts) = float_case(name)
    k = c["shape"][5]
    # the reference is resblock_cases' own
    t64, out64 = K.forward(c["x"], c["w0"], c["w2"], c["wsc"])
    assert np.array_equal(t64, ref["t"]) and np.array_equal(out64, ref["out"]) and K.same_bits(K.as_f32(t64), t32)
    kb = K.backward(c["x"], t32, out32, c["w0"], c["w2"], c["wsc"], c["g_out"])
    for key in ("g_x", "g_w0", "g_w2", "g_wsc"):
        assert (kb[key] is None and ref[key] is None) or np.array_equal(kb[key], ref[key]), key
    for key in K.OUTPUTS:
        assert ref[key] is None or (np.isfinite(ref[key]).all() and np.isfinite(bnd[key]).all() and (bnd[key] >= 0).all()), key
    assert 0.1 <= float((t32 > 0).mean()) <= 0.7 and (t32 == 0).any()       # (`border` leaves the middle of a map at zero)
    for key, (a, g, A) in parts.items():
        kk = 1 if key == "g_wsc" else k
        emu = G.emulate_wgrad(a, g, kk).reshape(A.shape).astype(np.float64)
        err = np.abs(emu - G.wgrad64(a, g, kk).reshape(A.shape))
        units = G.ratio(emu, emu - err, G.EPS * A)
        print("%s %-5s emulated error %.2f units of 2^-24 * A" % (name, key, units))
        assert units <= G.C_WGRAD / 2, (name, key, units)
        # ... and the bound of the restatement covers it at every element (for g_w0 the bound also carries gt's own)
        assert (err <= G.C_WGRAD * G.EPS * A).all() and (G.C_WGRAD * G.EPS * A <= bnd[key] * (1 + 1e-12)).all(), (name, key)


def test_emulation_is_exact_on_an_exact_case_and_ordered():
    """On integers the emulation equals float64; on float values it differs from a plain float32 sum in another order (it is an order)."""
    c, r = block("items3")
    gu = np.where(r["out"] > 0, c["g_out"], 0).astype(np.float32)
    assert np.array_equal(G.emulate_wgrad(K.as_f32(r["t"]), gu, 3).astype(np.float64), r["g_w2"])
    c, (t32, out32, ref, bnd, parts) = float_case("f_r_k5_24to8_positive")
    a, g, A = parts["g_w2"]
    emu = G.emulate_wgrad(a, g, 5)
    assert emu.dtype == np.float32 and not np.array_equal(emu.astype(np.float64), G.wgrad64(a, g, 5))


# ---- 4. the mask edges
@pytest.mark.parametrize("name", list(G.MASK_EDGES))
def test_mask_edges(name):
    c = G.make_block(name)
    r, worst = G.mask_edges_reference(c)
    assert worst < 2 ** 24
    values = [-G.SUB, 0.0, G.SUB, 2 * G.SUB]
    for key in ("t", "out"):
        a = c[key]
        assert a.dtype == np.float32 and set(np.unique(a).tolist()) == set(values)
        shares = [float((a == v).mean()) for v in values] + [float(np.signbit(a[a == 0]).mean())]
        assert 0.15 <= min(shares[0], shares[2], shares[3]) and 0.35 <= shares[1] <= 0.45 and 0.4 <= shares[4] <= 0.6, (key, shares)
    # the masks follow `> 0`: an element passes exactly where the caller's tensor is a positive subnormal
    k = c["shape"][5]
    gu = np.where(np.isin(c["out"], [np.float32(G.SUB), np.float32(2 * G.SUB)]), c["g_out"], np.float32(0))
    assert np.array_equal(G.wgrad64(c["t"], gu, k), r["g_w2"])
    assert c["wsc"] is None or np.array_equal(G.wgrad64(c["x"], gu, 1).reshape(c["wsc"].shape), r["g_wsc"])
    flipped = K.backward(c["x"], np.abs(c["t"]).astype(np.float64), c["out"], c["w0"], c["w2"], c["wsc"], c["g_out"])
    assert not np.array_equal(flipped["g_w0"], r["g_w0"]), "a mask of `!= 0` or `>= 0` on t would not show"
    # g_w2: exact subnormals, mostly non-zero; the others integers
    q = r["g_w2"] / G.SUB
    assert np.array_equal(q, np.rint(q)) and np.abs(r["g_w2"]).max() < 2.0 ** -126 and float((q != 0).mean()) > 0.9
    assert np.array_equal(K.as_f32(r["g_w2"]).astype(np.float64), r["g_w2"]), "as_f32 flushed a subnormal"
    for key in ("g_x", "g_w0", "g_wsc"):
        assert r[key] is None or (np.array_equal(r[key], np.rint(r[key])) and np.abs(r[key]).max() > 0), key


# ---- 5. the reference's own numbers on the new ground
def test_restatement_equals_golden():
    g17 = golden("g17_grad_sweep.npz")
    assert os.path.getsize(G.GOLDEN) < 1000000 and 0 < float(g17["max_abs"]) < 2 ** 24
    want = {}
    for name in G.IN_GOLDEN_BLOCKS:
        r = block(name)[1]
        want.update({"%s/%s" % (name, key): r[key] for key in ("g_x", "g_w0", "g_w2", "g_wsc") if r[key] is not None})
    for name in G.IN_GOLDEN_TRUNKS:
        r = G.trunk_exact(name)[1]
        want.update({"%s/%s" % (name, key): r[key] for key in T.golden_keys(r)})
    assert sorted(f for f in g17.files if f != "max_abs") == sorted(want)
    for key, v in want.items():
        assert g17[key].dtype in (np.int8, np.int32) and g17[key].shape == v.shape and np.array_equal(g17[key].astype(np.float64), v), key
