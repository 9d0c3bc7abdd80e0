"""CPU: the stem cases and their restatement (tests/stem_cases.py) against torch autograd, against the unified k x k convolution that
csrc/stem_train.hip computes, and against the reference's own numbers (tests/golden/g18_stem_grad.npz, written by
tools/gen_golden_stem.py from the four nets' padding_* and conv_* modules under autograd); the emulated order of additions against
the bounds; the two entry points in the library, the header and the ctypes table; the checks of a call on the CPU under a sanitizer."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import ROOT, golden
import stem_cases as S

NEW = ("pmp_stem_forward_device", "pmp_stem_backward_device")
CSRC = os.path.join(ROOT, "pmp_vvc_tip2023_amd", "csrc")


def d(a):
    return torch.from_numpy(np.asarray(a, np.float64).copy())


@pytest.mark.parametrize("name", list(S.EXACT))
def test_exact_case_fits_float32_in_any_order(name):
    c = S.make_case(name)
    n, h, w, cin, k, split = c["shape"]
    assert S.worst_partial_sum(c) < 2 ** 24
    for a in [c["x"], c["g_y"]] + c["w"] + c["b"]:
        assert a.dtype == np.float32 and np.array_equal(a, np.rint(a))
    assert c["x"].shape == (n, cin, h + k // 2, w + k // 2) and c["x"].min() >= 0 and 200 < c["x"][:, :cin - split].max() <= 255
    assert not split or c["x"][:, -1].max() == 3
    assert all(set(np.unique(wt)) == {-1.0, 1.0} for wt in c["w"]) and set(np.unique(c["g_y"])) == {-1.0, 0.0, 1.0}
    y = S.exact(name)[1]["y"]
    assert 0.25 < (y == 0).mean() < 0.75, "the zeros of y exercise the mask"
    gm_dropped = (c["g_y"] != 0) & (y == 0)
    assert gm_dropped.any() and ((c["g_y"] != 0) & (y > 0)).any()


def test_partition_cases_are_what_they_promise():
    assert [S.stem_np(S.EXACT["parts%d" % i]) for i in (1, 2, 3)] == [(1, 1), (2, 1), (3, 2)]
    assert S.stem_np(S.EXACT["cap_1023"]) == (1023, 512) and S.stem_np(S.EXACT["cap_1025"]) == (1025, 512)
    assert S.stem_np((64, 64, 64, 1, 5, 0)) == (1024, 512) and S.stem_np((200, 64, 64, 2, 9, 1)) == (3200, 512)
    src = open(os.path.join(CSRC, "stem_train.hip")).read()
    assert "(items + 1) / 2 < %d ? (items + 1) / 2 : %d" % (S.NP_CAP, S.NP_CAP) in src
    assert {S.EXACT[nm][3:] for nm in S.EXACT} >= {(1, 9, 0), (2, 9, 1), (3, 5, 0), (4, 5, 1), (4, 9, 1)}


@pytest.mark.parametrize("name", list(S.EXACT))
def test_restatement_equals_autograd(name):
    c = S.make_case(name)
    got, want = S.flat(S.restate(c)), S.autograd(c)
    assert sorted(got) == sorted(want)
    for key, v in want.items():
        assert got[key].shape == v.shape and np.array_equal(got[key], v), (name, key)


@pytest.mark.parametrize("name", list(S.FLOAT))
def test_float_restatement_is_close_to_autograd(name):
    c = S.make_case(*S.FLOAT[name])
    got, want = S.flat(S.restate(c)), S.autograd(c)
    for key, v in want.items():
        assert np.abs(got[key] - v).max() <= 1e-12 * max(1.0, np.abs(v).max()), (name, key)


@pytest.mark.parametrize("name", ["m_luma", "m_chroma", "parts2", "q_chroma"])
def test_split_restatement_equals_the_unified_convolution(name):
    """One k x k convolution with zero-padded kernels: the same y, g_x and - on the taps each kernel has - g_w; the taps it lacks get a
    gradient in the unified form, which must not leak into the output."""
    c = S.make_case(name)
    n, h, w, cin, k, split = c["shape"]
    p = k // 2
    want = S.flat(S.restate(c))
    wu, bu = S.unified(c["shape"], c["w"], c["b"])
    assert wu.shape == (32, cin, k, k) and bu.shape == (32,)
    assert np.array_equal(S.forward_unified(c), want["y"])
    x, wt, bt = d(c["x"]).requires_grad_(), d(wu).requires_grad_(), d(bu).requires_grad_()
    y = F.relu(F.conv2d(F.pad(x, (0, p, 0, p)), wt, bt))
    (y * d(c["g_y"])).sum().backward()
    g_w, g_b = S.split_grads(c["shape"], wt.grad.numpy(), bt.grad.numpy())
    got = S.flat({"y": y.detach().numpy(), "g_x": x.grad.numpy(), "g_w": g_w, "g_b": g_b})
    for key, v in want.items():
        assert np.array_equal(got[key], v), (name, key)
    if split:
        assert np.abs(wt.grad.numpy()[16:24, :, p + 1:, :]).max() > 0 and np.abs(wt.grad.numpy()[24:, :, :, p + 1:]).max() > 0
        assert not wu[16:24, :, p + 1:, :].any() and not wu[24:, :, :, p + 1:].any()


@pytest.mark.parametrize("name", S.IN_GOLDEN)
def test_restatement_equals_golden(name):
    g = golden("g18_stem_grad.npz")
    want = S.flat(S.restate(S.make_case(name)))
    assert sorted(k.split("/")[1] for k in g.files if k.startswith(name + "/")) == sorted(want)
    for key, v in want.items():
        assert np.array_equal(g["%s/%s" % (name, key)].astype(np.float64), v), (name, key)


def test_golden_is_small_and_below_2_to_24():
    g = golden("g18_stem_grad.npz")
    assert os.path.getsize(S.GOLDEN) < 1000000 and float(g["max_abs"]) < 2 ** 24
    assert sorted({k.split("/")[0] for k in g.files if "/" in k}) == sorted(S.IN_GOLDEN)


@pytest.mark.parametrize("name", list(S.FLOAT))
def test_emulated_order_stays_within_half_the_bound(name):
    c, y32, ref, bound, A = S.float_reference(name)
    emu = S.emulate(c, y32)
    assert sorted(emu) == sorted(ref)
    for key in ref:
        assert emu[key].dtype == np.float32 and emu[key].shape == ref[key].shape
        # (a bound of 0: an output channel that is dead on `pixels` - y = 0 on every pixel - whose gradients are exact zeros)
        assert np.isfinite(ref[key]).all() and (bound[key] >= 0).all() and (bound[key] > 0).any(), (name, key)
        r = S.ratio(emu[key], ref[key], bound[key])
        assert r <= 0.5, (name, key, r)
    assert S.C_FWD == 2 * S.C_FWD_EMULATED and S.C_WGRAD == 2 * S.C_WGRAD_EMULATED and S.C_DGRAD == 2 * S.C_DGRAD_EMULATED
    if S.FLOAT[name][1] == "positive":
        assert (c["x"] > 0).all() and (c["g_y"] > 0).all()


@pytest.mark.parametrize("name", ["parts3", "m_luma", "q_chroma"])
def test_emulation_is_exact_on_an_exact_case(name):
    c, want = S.exact(name)
    got = S.emulate(c, want["y"])
    for key, v in want.items():
        assert S.same_bits(got[key], v), (name, key)


def test_shape_of_refuses_what_is_not_a_stem():
    from pmp_vvc_tip2023_amd import stem
    z = lambda *s: torch.zeros(s)
    q = lambda cin=1, k=9, co=32: [(z(co, cin, k, k), z(co))]
    m = lambda cin=2, k=9: [(z(16, cin, k, k), z(16)), (z(8, cin, k // 2 + 1, k), z(8)), (z(8, cin, k, k // 2 + 1), z(8))]
    assert stem.shape_of(z(2, 1, 68, 36), q()) == (2, 64, 32, 1, 9, 0)
    assert stem.shape_of(z(3, 2, 20, 52), m()) == (3, 16, 48, 2, 9, 1)
    assert stem.shape_of(z(1, 3, 34, 34), q(3, 5)) == (1, 32, 32, 3, 5, 0)
    assert stem.shape_of(z(1, 4, 18, 34), m(4, 5)) == (1, 16, 32, 4, 5, 1)
    swapped = m()
    swapped[1], swapped[2] = swapped[2], swapped[1]
    bad = [(z(2, 1, 64, 64), q()), (z(2, 1, 68, 40), q()), (z(2, 1, 12, 20), q()), (z(2, 2, 68, 68), q()), (z(2, 1, 68, 68), q(1, 9, 16)),
           (z(2, 1, 68, 68), q(1, 7)), (z(2, 1, 66, 66), q(1, 3)), (z(2, 5, 68, 68), q(5)), (z(2, 2, 68, 68), swapped),
           (z(2, 2, 68, 68), m()[:2]), (z(2, 2, 68, 68), [m()[0]]), (z(2, 2, 68, 68), m(2, 5)[:1] + m()[1:]), (z(1, 68, 68), q()),
           (z(2, 2, 68, 68), [(w, None) for w, _ in m()]), (z(2, 2, 68, 68), [(w, z(4)) for w, _ in m()]),
           (z(2, 1, 68, 68), [(z(32, 1, 9, 9).reshape(32, 81), z(32))])]
    for x, convs in bad:
        with pytest.raises(ValueError):
            stem.shape_of(x, convs)


def test_entry_points_in_library_header_and_ctypes_table():
    from pmp_vvc_tip2023_amd import _lib, engine
    header = open(os.path.join(ROOT, "include", "pmp.h")).read()
    lib = _lib.load()
    for name in NEW:
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
        assert re.search(r"^int %s\(" % name, header, re.M), name
    assert "int n, h, w, cin, k, split;" in header
    assert [f[0] for f in _lib.StemShape._fields_] == ["n", "h", "w", "cin", "k", "split"] and C.sizeof(_lib.StemShape) == 24
    s = _lib.stem_shape((3, 48, 16, 2, 9, 1))
    assert (s.n, s.h, s.w, s.cin, s.k, s.split) == (3, 48, 16, 2, 9, 1) and _lib.stem_shape(s) is s
    assert len(_lib.SIGNATURES["pmp_stem_forward_device"][1]) == 6 and len(_lib.SIGNATURES["pmp_stem_backward_device"][1]) == 9
    assert callable(engine.Engine.stem_forward_device) and callable(engine.Engine.stem_backward_device)
    for src in ("Makefile", os.path.join("..", "..", "tools", "abl", "Makefile")):
        assert "stem_train" in open(os.path.join(CSRC, src)).read(), src


def test_train_check_passes_with_the_stem_matrix():
    """train_check.h with a main of its own under AddressSanitizer and UBSan: a stand-alone CPU program, built and run once."""
    r = subprocess.run(["make", "-s", "-C", CSRC, "traincheck"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "train_check: ok" in r.stdout, (r.stdout + r.stderr)[-2000:]
    assert "stem_shape_ok" in open(os.path.join(CSRC, "train_check_main.cpp")).read()
