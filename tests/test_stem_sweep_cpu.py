"""CPU: the reach and the fitness of the stem's sweep (tests/stem_sweep_cases.py): every exact case fits float32 in any order and its
restatement equals autograd; the table holds all sixteen (cin, k, split) at two shapes each, every NT, the cap of the partition with
the wide accumulator sets, a four-item workgroup, sides and n of 256; the mask-edge and 2^-149 cases are what they promise; the
emulated order of additions stays within half of each float bound, and the constants are what the emulation gives."""
import numpy as np
import pytest

import stem_cases as S
import stem_sweep_cases as W

UNITS = {}                                         # kernel -> (largest emulated error in units of 2^-24 A, case, output)


# ---- 1. every exact case: what test_exact_case_fits_float32_in_any_order asserts, and the restatement against autograd
@pytest.mark.parametrize("name", list(W.EXACT))
def test_exact_case_fits_float32_and_equals_autograd(name):
    c, want = W.exact(name)
    n, h, w, cin, k, split = c["shape"]
    assert c["shape"] == W.EXACT[name]
    assert S.worst_partial_sum(c) < 2 ** 24
    for a in [c["x"], c["g_y"]] + c["w"] + c["b"]:
        assert a.dtype == np.float32 and np.array_equal(a, np.rint(a))
    assert c["x"].shape == (n, cin, h + k // 2, w + k // 2) and c["x"].min() >= 0
    assert cin == split or 200 < c["x"][:, :cin - split].max() <= 255          # (cin = 1, split: the only channel is the QT map)
    assert not split or c["x"][:, -1].max() == 3
    assert all(set(np.unique(wt)) == {-1.0, 1.0} for wt in c["w"]) and set(np.unique(c["g_y"])) == {-1.0, 0.0, 1.0}
    assert (name in W.SPARSE) == ((c["g_y"] != 0).mean() < 0.1)
    y = want["y"]
    assert 0.25 < (y == 0).mean() < 0.75, "the zeros of y exercise the mask"
    assert ((c["g_y"] != 0) & (y == 0)).any() and ((c["g_y"] != 0) & (y > 0)).any()
    ref = S.autograd(c)
    assert sorted(ref) == sorted(want)
    for key, v in ref.items():
        assert want[key].dtype == np.float32 and want[key].shape == v.shape and np.array_equal(want[key].astype(np.float64), v), (name, key)


# ---- 2. the reach, from the table
def test_the_table_reaches_what_it_promises():
    for prefix, nhw in (("one", (1, 16, 16)), ("two", (2, 32, 48))):
        got = sorted(s[3:] for nm, s in W.EXACT.items() if nm.startswith(prefix + "_"))
        assert got == sorted(W.TRIPLES) and all(W.EXACT[nm][:3] == nhw for nm in W.EXACT if nm.startswith(prefix + "_"))
    assert len(W.TRIPLES) == len(set(W.TRIPLES)) == 16
    assert set(W.TRIPLES) == {(cin, k, split) for cin in range(1, 5) for k in (5, 9) for split in (0, 1)}
    assert len(W.EXACT) == 32 + 5 + 5 and not set(W.EXACT) & set(S.EXACT)
    assert S.stem_np((1, 16, 16, 1, 5, 0)) == (1, 1) and S.stem_np((2, 32, 48, 1, 5, 0)) == (12, 6)
    assert W.items_per_workgroup((2, 32, 48, 1, 5, 0)) == (2, 2)
    assert {W.nt(s) for nm, s in W.EXACT.items() if nm.startswith("two_")} == {2, 4, 5, 6, 7, 11, 16, 21}
    assert W.nt(W.EXACT["two_c3k9s0"]) == 16 and W.nt(W.EXACT["two_c2k5s1"]) == 4
    # the partition
    assert {nm: S.stem_np(W.EXACT[nm]) for nm in W.PARTITION} == W.PROMISED
    assert W.PROMISED == {"parts4": (4, 2), "parts5": (5, 3), "cap_luma": (1040, 512), "cap_wide": (1024, 512), "four": (1540, 512)}
    assert W.nt(W.EXACT["cap_luma"]) == 11 and W.nt(W.EXACT["cap_wide"]) == 21
    assert W.items_per_workgroup(W.EXACT["cap_luma"]) == (3, 2) and 1040 - 2 * 512 == 16
    assert W.items_per_workgroup(W.EXACT["cap_wide"]) == (2, 2)
    assert W.items_per_workgroup(W.EXACT["four"]) == (4, 3) and 1540 - 3 * 512 == 4
    assert W.items_per_workgroup(W.EXACT["parts5"]) == (2, 1)
    # the extents of include/pmp.h
    assert max(s[0] for s in W.EXACT.values()) == 256 and max(s[1] for s in W.EXACT.values()) == 256
    assert max(s[2] for s in W.EXACT.values()) == 256
    assert W.EXTENTS["x256"][:3] == W.EXTENTS["luma256"][:3] == (1, 256, 256) and W.EXTENTS["luma256"][3:] == (2, 9, 1)
    assert W.EXTENTS["tall"][1:3] == (256, 16) and W.EXTENTS["wide"][1:3] == (16, 256) and W.EXTENTS["n256"][:3] == (256, 16, 16)
    for nm in ("x256", "luma256"):                 # the input gradient's seventeenth tile row and column hold k/2 lines
        n, h, w, cin, k, split = W.EXTENTS[nm]
        assert (h + k // 2 + 15) // 16 == 17 and h + k // 2 - 256 == k // 2
    # the arena and stem.py cases
    assert sorted(s[3:] for s in W.ARENA.values()) == [(1, 5, 0), (2, 9, 0), (3, 9, 1), (4, 5, 1), (4, 9, 1)]
    assert all(S.stem_np(s)[0] >= 2 for s in list(W.ARENA.values()) + list(W.MASK_EDGES.values()))
    assert list(W.STEM_PY.values()) == [(2, 32, 16, 2, 9, 1), (2, 16, 32, 3, 5, 0)]
    assert {s[4:] for s in W.MASK_EDGES.values()} == {(9, 1), (5, 0)}


# ---- 3. masks on the edge of `> 0`, and the cases times 2^-149
@pytest.mark.parametrize("name", list(W.MASK_EDGES))
def test_mask_edge_cases(name):
    c, y, want = W.mask_edges(name)
    assert y.dtype == np.float32 and y.shape == c["g_y"].shape
    bits = y.view(np.uint32)
    assert sorted(np.unique(bits)) == sorted(W.MASK_VALUES.view(np.uint32)) and len(np.unique(bits)) == 6
    for co in range(32):
        assert len(np.unique(bits[:, co])) == 6, "every output channel sees every value"
    assert 0.4 < (y > 0).mean() < 0.6
    for a in [c["x"], c["g_y"]] + c["w"]:
        assert np.array_equal(a, np.rint(a))
    a = S.backward(c, y, absolute=True)
    assert max([float(a["g_x"].max())] + [float(v.max()) for v in a["g_w"] + a["g_b"]]) < 2 ** 24
    # against autograd's own rule on the float32 y: relu's gradient passes where its OUTPUT is above zero
    import torch
    yt = torch.from_numpy(y.astype(np.float64)).requires_grad_()
    (torch.relu(yt) * torch.from_numpy(c["g_y"].astype(np.float64))).sum().backward()
    gm = np.where(y > 0, c["g_y"], np.float32(0)).astype(np.float64)
    assert np.array_equal(yt.grad.numpy(), gm)
    assert np.array_equal(want["g_b0"], gm[:, :len(want["g_b0"])].sum((0, 2, 3)).astype(np.float32))
    for k, v in want.items():
        assert np.abs(v).max() > 0, k


@pytest.mark.parametrize("which", ["x_tiny", "g_tiny"])
@pytest.mark.parametrize("name", list(W.TINY))
def test_tiny_cases_are_the_exact_case_times_2_to_minus_149(name, which):
    c, want, base = W.tiny(name, which)
    assert S.worst_partial_sum(S.make_case(name, shape=W.TINY[name])) < 2 ** 24, "every partial sum below 2^24 units of 2^-149"
    assert 1 <= S.stem_np(c["shape"])[0] <= 2
    scaled = W.scaled_outputs(c, which)
    assert sorted(want) == sorted(base)
    nonzero = below = 0
    for key, v in want.items():
        f = W.TINY_SCALE if key in scaled else 1.0
        assert np.array_equal(v.astype(np.float64), base[key] * f), (name, which, key)
        assert np.abs(v).max() > 0, key
        if key in scaled:
            nonzero += int((v != 0).sum())
            below += int(((v != 0) & (np.abs(v) < 2.0 ** -126)).sum())
    assert below > 0.9 * nonzero, (below, nonzero)
    assert np.array_equal(want["y"] > 0, base["y"] > 0), "the mask is the unscaled case's"


# ---- 4. float cases: the emulated order within half of each bound; the constants are made of its figures
@pytest.mark.parametrize("name", list(W.FLOAT))
def test_emulated_order_stays_within_half_the_bound(name):
    c, y32, ref, bound, A = W.float_reference(name)
    emu = S.emulate(c, y32)
    assert sorted(emu) == sorted(ref)
    for key in ref:
        assert emu[key].dtype == np.float32 and emu[key].shape == ref[key].shape
        assert np.isfinite(ref[key]).all() and (bound[key] >= 0).all() and (bound[key] > 0).any(), (name, key)
        r, u = S.ratio(emu[key], ref[key], bound[key]), W.units(emu[key], ref[key], A[key])
        kernel = W.KERNEL_OF(key)
        if u > UNITS.get(kernel, (0.0,))[0]:
            UNITS[kernel] = (u, name, key)
        print("%-16s %-5s emulated |err| = %.2f units of 2^-24 A, %.3f of the bound" % (name, key, u, r))
        assert r <= 0.5, (name, key, r)
        assert u <= {"forward": W.C_FWD_EMULATED, "wgrad": W.C_WGRAD_EMULATED, "dgrad": W.C_DGRAD_EMULATED}[kernel]
    if W.FLOAT[name][1] == "positive":
        assert (c["x"] > 0).all() and (c["g_y"] > 0).all()


def test_constants_come_from_the_emulation():
    """(after the cases above, in file order) each constant is the larger of stem_cases' and twice the emulated figure, and the
    emulated figure written down is the one reached, rounded up in its last digit."""
    assert W.C_FWD == max(S.C_FWD, 2 * W.C_FWD_EMULATED) and W.C_WGRAD == max(S.C_WGRAD, 2 * W.C_WGRAD_EMULATED)
    assert W.C_DGRAD == max(S.C_DGRAD, 2 * W.C_DGRAD_EMULATED)
    assert (S.C_FWD, S.C_WGRAD, S.C_DGRAD) == (14.0, 25.0, 15.4), "the old table keeps its constants"
    if len(UNITS) == 3:                            # the whole file ran
        for kernel, written in (("forward", W.C_FWD_EMULATED), ("wgrad", W.C_WGRAD_EMULATED), ("dgrad", W.C_DGRAD_EMULATED)):
            print("%-8s emulated %.3f (%s, %s); written %.2f" % ((kernel,) + UNITS[kernel] + (written,)))
            assert written - 0.1 <= UNITS[kernel][0] <= written, (kernel, UNITS[kernel], written)
    assert W.FLOAT_SHAPES == {"f_q49": (2, 32, 16, 4, 9, 0), "f_m15": (3, 16, 32, 1, 5, 1), "f_m39": (1, 32, 32, 3, 9, 1),
                              "f_q25": (2, 16, 48, 2, 5, 0), "f_parts": (8, 64, 64, 2, 9, 1)}
    assert S.stem_np(W.FLOAT_SHAPES["f_parts"]) == (128, 64) and len(W.FLOAT) == 15
