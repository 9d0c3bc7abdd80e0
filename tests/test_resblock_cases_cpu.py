"""CPU: the ResidualBlock cases and their restatement (tests/resblock_cases.py) against the reference's own numbers
(tests/golden/g15_resblock_grad.npz, written by tools/gen_golden_resblock.py from Model_QBD.ResidualBlock under autograd), and the four
entry points in the header and the ctypes table."""
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT, golden
import resblock_cases as K

NEW = ("pmp_resblock_forward", "pmp_resblock_forward_device", "pmp_resblock_backward", "pmp_resblock_backward_device")


@pytest.fixture(scope="module")
def g15():
    return golden("g15_resblock_grad.npz")


@pytest.mark.parametrize("name", K.IN_GOLDEN)
def test_restatement_equals_reference(g15, name):
    """Exactly, in float64 and in float32: on these integers every float32 operation is exact, whatever the order of summation."""
    c = K.make_exact(name)
    r64, r32 = K.restate(c, torch.float64), K.restate(c, torch.float32)
    for key in K.OUTPUTS:
        stored = "%s_%s" % (name, key)
        if r64[key] is None:
            assert key == "g_wsc" and c["wsc"] is None and stored not in g15.files
            continue
        if (name, key) in K.NOT_STORED:
            assert stored not in g15.files
        else:
            ref = g15[stored]
            assert ref.dtype in (np.int8, np.int32) and ref.shape == r64[key].shape, (name, key)
            assert np.array_equal(ref.astype(np.float64), r64[key]), (name, key)
        assert r32[key].dtype == np.float32 and np.array_equal(r32[key].astype(np.float64), r64[key]), (name, key, "float32 is not exact")
        assert K.same_bits(K.as_f32(r64[key]), r32[key] + np.float32(0)), (name, key)


def test_golden_is_small_and_below_2_to_24(g15):
    assert os.path.getsize(K.GOLDEN) < 1000000
    assert 0 < float(g15["max_abs"]) < 2 ** 24
    assert sorted({f.rsplit("_g_", 1)[0].rsplit("_t", 1)[0].rsplit("_out", 1)[0] for f in g15.files if f != "max_abs"}) == sorted(K.IN_GOLDEN)


@pytest.mark.parametrize("name", list(K.EXACT))
def test_exact_cases_are_integers_with_zeros_and_both_signs(name):
    c = K.make_exact(name)
    n, h, w, cin, cout, k = c["shape"]
    assert c["x"].shape == (n, cin, h, w) and np.abs(c["x"]).max() == 2 and set(np.unique(c["w0"])) == {-1.0, 0.0, 1.0}
    assert (c["wsc"] is None) == (cin == cout)
    t, out = K.forward(c["x"], c["w0"], c["w2"], c["wsc"])
    for a in (t, out):
        assert np.array_equal(a, np.rint(a)) and (a == 0).any() and 0.3 < (a > 0).mean() < 0.7
    # whatever order a float32 kernel adds in, no partial sum leaves the integers float32 holds exactly
    assert K.worst_partial_sum(c) < 2 ** 24


def test_float_cases_fix_the_masks():
    """t and out of a float case reach the backward pass as float32 roundings of the float64 forward: a float32 forward differs from
    them in the last bits, which is why the backward pass takes them from the caller."""
    c = K.make_float("f_c64_32")
    t64, out64 = K.forward(c["x"], c["w0"], c["w2"], c["wsc"])
    t32, out32 = K.forward(c["x"], c["w0"], c["w2"], c["wsc"], torch.float32)
    assert K.rel_err(t32, t64) < 1e-5 and K.rel_err(out32, out64) < 1e-5
    r = K.backward(c["x"], K.as_f32(t64), K.as_f32(out64), c["w0"], c["w2"], c["wsc"], c["g_out"])
    assert r["g_x"].shape == c["x"].shape and r["g_wsc"].shape == c["wsc"].shape and np.isfinite(r["g_w0"]).all()


def test_entry_points_in_header_and_ctypes_table():
    from pmp_vvc_tip2023_amd import _lib
    header = open(os.path.join(ROOT, "include", "pmp.h")).read()
    for name in NEW:
        assert name in _lib.SIGNATURES, name
        assert re.search(r"^int %s\(pmp_ctx \*ctx, const pmp_rb_shape \*shape," % name, header, re.M), name
    assert [f[0] for f in _lib.RbShape._fields_] == ["n", "h", "w", "cin", "cout", "k"]
    assert re.search(r"typedef struct pmp_rb_shape \{\s*int n, h, w, cin, cout, k;\s*\} pmp_rb_shape;", header)
    assert len(_lib.SIGNATURES["pmp_resblock_forward_device"][1]) == 8 and len(_lib.SIGNATURES["pmp_resblock_backward_device"][1]) == 13
