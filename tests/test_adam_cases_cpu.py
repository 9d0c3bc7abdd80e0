"""CPU: the restatements of pmp_adam_step_device (tests/adam_cases.py) against torch.optim.Adam(foreach=False) on the CPU, and the new
symbols in the header, the ctypes table and the library.

float64: adam64 equals torch's float64 Adam to rounding over 3 steps, sizes 1 .. 204 800 and gradient scales 1e-3 .. 1e3.  The bounds
are float64 rounding at the values' magnitudes, eight times 2.2e-16 relative: parameters are O(1), m is of the gradient's scale, v of
its square (1.8e-9 at scale 1e3, where torch's v was seen to lie 3.6e-12 away).
float32: adam32, include/pmp.h's order of operations, satisfies the GPU test's bound against the same torch runs.  How many elements
differ from torch's bits is printed, not asserted: torch's float32 CPU kernels give different bits on different CPUs (3 to 29 of
619 605 elements differed where this was written, numpy's double-rounded stand-in for fma accounting for some)."""
import os
import re

import numpy as np
import pytest
import torch

import adam_cases as A
from conftest import ROOT


@pytest.mark.parametrize("scale", A.SCALES)
def test_float64_restatement_equals_torch_float64_adam(scale):
    t = A.tensors(A.SIZES, 100, scale)
    want, _ = A.torch_adam(t, 3, torch.float64)
    got = A.run(A.adam64, t, 3)
    eps64 = 2.2e-16
    for key, tol in (("param", 8 * eps64), ("m", 8 * eps64 * max(scale, 1.0)), ("v", 8 * eps64 * max(scale * scale, 1.0))):
        for a, b in zip(got[key], want[key]):
            d = float(np.abs(a - b).max())
            print("scale %g %s n %d: %.3g" % (scale, key, a.size, d))
            assert d <= tol, (key, a.size, d)


@pytest.mark.parametrize("first_step,state", [(1, False), (1000, True)])
@pytest.mark.parametrize("scale", A.SCALES)
def test_header_order_in_float32_meets_the_bound(scale, first_step, state):
    t = A.tensors(A.SIZES, 7, scale, zeros=scale == 1.0, state=state)
    steps = 1 if state else 3
    t32, _ = A.torch_adam(t, steps, torch.float32, first_step)
    r64 = A.run(A.adam64, t, steps, first_step)
    got = A.run(A.adam32, t, steps, first_step)
    print("worst distance / bound: %.3f" % A.check_bound("adam32", got, t32, r64, A.peaks(t, steps, first_step)))
    total = sum(a.size for a in got["param"])
    differ = sum(int((a != b).sum()) for key in got for a, b in zip(got[key], t32[key]))
    print("elements that differ from torch's float32 bits: %d of %d" % (differ, 3 * total))   # a figure: torch's bits depend on the CPU


def test_nonfinite_gradients_give_torchs_pattern_in_the_restatement():
    t = A.nonfinite_case()
    t32, _ = A.torch_adam(t, 1, torch.float32, 5)
    got = A.run(A.adam32, t, 1, 5)
    for key in got:
        assert np.array_equal(A.pattern(got[key][0]), A.pattern(t32[key][0])), key
        fin = A.pattern(t32[key][0]) == 0
        assert fin.sum() == 6 and np.array_equal(got[key][0][fin], t32[key][0][fin]), key
    assert np.array_equal(A.pattern(got["param"][0])[[1, 4, 7]], [1, 1, 1]) and np.array_equal(A.pattern(got["m"][0])[[1, 4, 7]], [1, 2, 3])


def test_the_lists_are_what_the_issue_names():
    L = A.lists()
    assert len(L["joint"]) == 92 and min(L["joint"]) == 1 and 1500000 < sum(L["joint"]) < 1600000
    assert len(L["ones"]) == 300 and L["sizes"] == [1, 2, 3, 63, 64, 65, 255, 257, 1025, 204800]


def test_new_symbols_in_header_table_and_library():
    from pmp_vvc_tip2023_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "pmp.h")).read()
    assert "TRAINING STEP" in hdr
    lib = _lib.load()
    for name in ("pmp_batch_gather_device", "pmp_adam_step_device"):
        assert re.search(r"\bint %s\(pmp_ctx \*ctx" % name, hdr) and name in _lib.SIGNATURES and hasattr(lib, name), name
    assert re.search(r"#define PMP_ADAM_TABLE %d\b" % _lib.PMP_ADAM_TABLE, hdr) and re.search(r"#define PMP_BATCH_MAX %d\b" % _lib.PMP_BATCH_MAX, hdr)
    # the kernel's argument block: the table of PMP_ADAM_TABLE entries (four pointers, a count, a first workgroup) stays under 4 KB
    assert _lib.PMP_ADAM_TABLE * (4 * 8 + 4 + 4) + 64 <= 4096
