"""CPU: the numpy restatement of pmp_batch_gather_device (tests/batch_cases.py) against what Metrics.Load_Pre_VP_Dataset's statements
build with torch on the CPU, luma and chroma, the uint8 wrap of a raw qtDepth 0 to 255.0 included, and its out-of-range rule."""
import numpy as np
import pytest

import batch_cases as B


@pytest.mark.parametrize("chroma", [False, True], ids=["Luma", "Chroma"])
@pytest.mark.parametrize("which", list(B.indices()))
def test_restatement_equals_the_loaders_statements(which, chroma):
    d, index = B.dataset(), B.indices()[which]
    got, status = B.gather(d, index, chroma)
    want = B.loader_rows(d, index, chroma)
    assert status == 0 and got["x"].shape == ((len(index), 3, 34, 34) if chroma else (len(index), 1, 68, 68))
    for k, w in want.items():
        assert got[k].shape == w.shape and np.array_equal(got[k].astype(np.float32), w), k
    assert got["x"].dtype == np.float32 and got["qt_f"].dtype == np.float32 and got["qt8"].dtype == np.uint8 and got["msdire"].dtype == np.int8


def test_a_raw_zero_wraps_to_255():
    d = B.dataset()
    assert d["qt8"][0, 0, 0] == 0
    got, _ = B.gather(d, [0], False)
    assert got["qt_f"][0, 0, 0, 0] == 255.0 and B.loader_rows(d, [0], False)["qt_f"][0, 0, 0, 0] == 255.0


def test_rows_outside_the_set_are_zeros_and_raise_the_status_bit():
    d = B.dataset()
    got, status = B.gather(d, [2, -1, B.N, 2], True)
    clean, _ = B.gather(d, [2], True)
    assert status == 1
    for k in B.KEYS:
        assert not got[k][1].any() and not got[k][2].any() and np.array_equal(got[k][0], clean[k][0]) and np.array_equal(got[k][3], clean[k][0]), k
