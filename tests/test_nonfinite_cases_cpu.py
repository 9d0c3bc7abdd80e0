"""CPU: conditions on the table of tests/nonfinite_cases.py that make tests/test_gpu_nonfinite.py a real check.  They hold for the
torch reference alone; a case that breaks one is changed, the condition stays."""
import functools

import numpy as np
import pytest
import torch

import nonfinite_cases as NF


@functools.lru_cache(maxsize=None)
def footprint(name, dtype):
    return NF.footprints(NF.reference(NF.make(name), dtype))


def weight_gradients(r):
    return [k for k in r if k.startswith("g_w") or k.startswith("g_b")]


def test_the_table_holds_what_the_contract_names():
    for family, shapes in NF.SHAPES.items():
        for shape in shapes:
            assert shape[0] >= 2
            got = NF.plants_of(family, shape)
            assert {"nan_corner", "nan_seam", "pinf", "ninf", "pair", "g", "w0", "w2", "overflow"} <= set(got)
            assert ("pool_last" in got) == NF.has_pool(family, shape)
    for name in NF.CASES:
        assert all(idx[0] == 0 for nm, idx, _ in NF.plants(name) if NF.is_data_plant(name)), "image 1 stays free of plants"


def test_make_plants_exactly_the_listed_elements():
    for name in NF.CASES:
        a, b = NF.clean(name), NF.make(name)
        changed = 0
        for (nm, u), (_, v) in zip(NF._weights(a["family"], a) + [(k, a[k]) for k in (NF.X_OF[a["family"]], NF.G_OF[a["family"]])],
                                   NF._weights(b["family"], b) + [(k, b[k]) for k in (NF.X_OF[b["family"]], NF.G_OF[b["family"]])]):
            changed += int((u.view(np.uint32) != v.view(np.uint32)).sum())
        assert changed == len(NF.plants(name)), name


@pytest.mark.parametrize("name", list(NF.CASES))
def test_case_conditions(name):
    family, shape, plant = NF.CASES[name]
    R = footprint(name, NF.reference_dtype(name))
    S = NF.reach(name)
    assert sorted(R) == sorted(S)
    # R inside S: the reach is a reach
    for k in R:
        assert R[k].shape == S[k].shape and not (R[k] & ~S[k]).any(), (name, k, "R outside S")
    # containment is a real check: S covers at most half of every data tensor
    if NF.is_data_plant(name):
        for k in S:
            if k not in weight_gradients(S):
                assert S[k].mean() <= 0.5, (name, k, S[k].mean())
                assert not S[k][1:].any(), (name, k, "the second image is reachable")
    # detection is a real check: a plant in x shows in t, in the output and in a weight gradient; one in g, in g_x and a weight gradient.
    # A plant in a WEIGHT is held to the output only: w2 and wsc lie behind t, and torch's threshold_backward hands the finite gradient
    # on where the output is NaN, so that no weight gradient need be non-finite (a stem's are not).
    if plant in NF.DATA_PLANTS:
        firsts = {"block": ("t0", "y"), "trunk": ("t0", "y"), "qtail": ("s1", "x9"), "stem": ("y",)}[family]
        for k in firsts:
            assert R[k].any(), (name, k, "torch reports nothing here")
        assert any(R[k].any() for k in weight_gradients(R)), (name, "no weight gradient")
    elif plant in NF.WEIGHT_PLANTS:
        assert R[NF.Y_OF[family]].any(), (name, "torch reports nothing in the output")
        if plant == "w0" and family != "stem":           # in front of t: there the issue's whole condition holds
            assert R["s1" if family == "qtail" else "t0"].any() and any(R[k].any() for k in weight_gradients(R)), name
    else:
        assert R[NF.G_X[family]].any() and any(R[k].any() for k in weight_gradients(R)), name
    # the footprint does not depend on the precision, except where the inf is born by float32 overflow
    if plant != "overflow":
        R32 = footprint(name, torch.float32)
        for k in R:
            assert np.array_equal(R[k], R32[k]), (name, k, "float32 and float64 footprints differ")
    else:
        R64 = footprint(name, torch.float64)
        assert not any(v.any() for v in R64.values()), (name, "float64 overflows too")


def test_the_hand_placed_g_plants_are_what_the_search_finds():
    for (family, shape), at in NF.G_AT.items():
        assert NF.find_g_at(family, shape) == at, (family, shape, "qtail_cases' values changed: take find_g_at's element")


def test_minus_inf_is_not_plus_inf():
    """relu(-inf) = 0: the two signs leave different footprints in t, so neither case stands for the other."""
    for family, shapes in NF.SHAPES.items():
        a, b = (footprint(NF.case_id(family, shapes[0], p), torch.float64) for p in ("pinf", "ninf"))
        k = {"qtail": "s1", "stem": "y"}.get(family, "t0")
        assert not np.array_equal(a[k], b[k]), family


# ---- the heads and the gate
@functools.lru_cache(maxsize=None)
def head_footprint(name, dtype):
    return {k: None if v is None else ~np.isfinite(v) for k, v in NF.head_reference(NF.head_make(name), dtype).items()}


def test_head_reference_is_head_cases_restatement_on_clean_values():
    """the autograd form and head_cases' written-out formulas are the same function where everything is finite"""
    for nm in NF.HEAD_SHAPES:
        c = NF.head_clean("head-%s-g" % nm)
        a, b = NF.head_reference(c), NF.H.restate(c)
        for k in NF.H.OUT_KEYS:
            if a[k] is None:
                assert b[k] is None or k in ("g_prev", "g_q"), (nm, k)
            else:
                assert np.abs(a[k] - b[k]).max() <= 1e-12 * max(1.0, np.abs(b[k]).max()), (nm, k)


@pytest.mark.parametrize("name", list(NF.HEAD_CASES))
def test_head_case_conditions(name):
    nm, plant = NF.HEAD_CASES[name]
    R, R32, S = head_footprint(name, torch.float64), head_footprint(name, torch.float32), NF.head_reach(name)
    for k in NF.H.OUT_KEYS:
        assert (R[k] is None) == (S[k] is None), (name, k)
        if R[k] is None:
            continue
        assert not (R[k] & ~S[k]).any(), (name, k, "R outside S")
        assert np.array_equal(R[k], R32[k]), (name, k, "float32 and float64 footprints differ")
        if plant not in ("w", "b") and k not in ("g_w", "g_b"):
            assert S[k].mean() <= 0.5, (name, k, S[k].mean())
            assert not S[k][1:].any(), (name, k, "another image is reachable")
    # detection is a real check: where a plant must show under torch (a plant in x: in y and in the weight gradient)
    seen = {"q": ("att",), "g": ("g_x", "g_w", "g_b"), "g_att": ("g_x", "g_w", "g_b"), "w": ("y", "g_x"), "b": ("y",),
            "prev": ("y",)}.get(plant, ("y", "g_w"))
    for k in seen:
        assert R[k].any(), (name, k, "torch reports nothing here")


def test_gate_table():
    for count, at in NF.GATE_COUNTS.items():
        assert at == count - 1 and (count == 1 or count % 256 in (255, 1))
        for key, value in NF.GATE_PLANTS:
            c, reads = NF.gate_make(count, key, value)
            want = NF.H.gate_reference(c, True)
            for k, v in want.items():
                bad = ~np.isfinite(v)
                assert bad[:at].sum() == 0 and bool(bad[at]) == (k in reads), (count, key, value, k)
