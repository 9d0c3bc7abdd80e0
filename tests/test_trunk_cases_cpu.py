"""CPU: the trunk cases and their restatement (tests/trunk_cases.py) against torch autograd and against the reference's own numbers
(tests/golden/g16_trunk_grad.npz, written by tools/gen_golden_trunk.py from Model_QBD.ResidualBlock modules in an nn.Sequential with
F.max_pool2d under autograd), and the four entry points in the library, the header and the ctypes table."""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import ROOT, golden
import resblock_cases as K
import trunk_cases as T

NEW = ("pmp_trunk_saved_bytes", "pmp_trunk_forward_device", "pmp_trunk_backward_device", "pmp_trunk_unpack_device")


@functools.lru_cache(maxsize=None)
def case(name):
    """-> (case, float64 restatement); computed once, never changed."""
    c = T.make_exact(name)
    return c, T.restate(c)


def autograd(c):
    """The trunk as float64 torch ops under autograd, the way nn.Sequential of ResidualBlocks and F.max_pool2d compute it."""
    d = lambda a: torch.from_numpy(np.asarray(a, np.float64).copy())
    x = d(c["x"]).requires_grad_()
    ws, ts, outs = [], [], []
    a = x
    for w0, w2, wsc in c["blocks"]:
        w = [d(w0).requires_grad_(), d(w2).requires_grad_(), None if wsc is None else d(wsc).requires_grad_()]
        p = w0.shape[2] // 2
        t = F.relu(F.conv2d(a, w[0], padding=p))
        a = F.relu(F.conv2d(t, w[1], padding=p) + (a if wsc is None else F.conv2d(a, w[2].reshape(*w[2].shape, 1, 1))))
        ws.append(w); ts.append(t); outs.append(a)
    y = F.max_pool2d(a, 2) if c["shape"][5] else a
    (y * d(c["g_y"])).sum().backward()
    num = lambda v: None if v is None else v.detach().numpy()
    return {"y": num(y), "g_x": num(x.grad), "t": [num(t) for t in ts], "out": [num(o) for o in outs],
            "g_w": [tuple(None if v is None else num(v.grad) for v in w) for w in ws]}


@pytest.mark.parametrize("name", list(T.EXACT))
def test_bound_below_2_to_24_and_ties_present(name):
    c, r = case(name)
    n, h, w, cin, blocks, pool = c["shape"]
    assert c["x"].shape == (n, cin, h, w) and np.abs(c["x"]).max() == 2 and c["g_y"].shape == T.y_shape(c["shape"])
    for (ci, co, k), (w0, w2, wsc) in zip(T.block_shapes(c["shape"]), c["blocks"]):
        assert w0.shape == (co, ci, k, k) and w2.shape == (co, co, k, k) and (wsc is None) == (ci == co)
        assert set(np.unique(w0)) == {-1.0, 0.0, 1.0} and set(np.unique(w2)) == {-1.0, 0.0, 1.0}
    for a in r["t"] + r["out"]:
        assert np.array_equal(a, np.rint(a)) and (a == 0).any() and (a > 0).any()
    # whatever order a float32 kernel adds in, no partial sum leaves the integers float32 holds exactly
    assert T.worst_partial_sum(c) < 2 ** 24
    if pool:
        assert T.tied_positive_windows(r["out"][-1]) >= 1, "the first-maximum rule is not exercised"


@pytest.mark.parametrize("name", list(T.EXACT))
def test_restatement_equals_autograd(name):
    """Exactly, ties included, in float64; and a float32 evaluation of the restatement is exact too."""
    c, r = case(name)
    ref, r64, r32 = T.flat(autograd(c)), T.flat(r), T.flat(T.restate(c, torch.float32))
    assert sorted(ref) == sorted(r64) == sorted(r32)
    for key in ref:
        assert ref[key].shape == r64[key].shape and np.array_equal(ref[key], r64[key]), (name, key)
        assert r32[key].dtype == np.float32 and np.array_equal(r32[key].astype(np.float64), r64[key]), (name, key, "float32 is not exact")


def test_pool_backward_takes_the_first_maximum():
    a = np.zeros((1, 1, 2, 8))
    a[0, 0, :, 0:2] = [[3, 3], [3, 3]]         # all four tie: (0,0)
    a[0, 0, :, 2:4] = [[1, 2], [2, 0]]         # (0,1) and (1,0) tie: (0,1)
    a[0, 0, :, 4:6] = [[0, 1], [5, 5]]         # (1,0) and (1,1) tie: (1,0)
    a[0, 0, :, 6:8] = [[0, 0], [0, 7]]         # no tie: (1,1)
    g = np.array([[[[10.0, 20.0, 30.0, 40.0]]]])
    want = np.zeros_like(a)
    want[0, 0, 0, 0], want[0, 0, 0, 3], want[0, 0, 1, 4], want[0, 0, 1, 7] = 10, 20, 30, 40
    assert np.array_equal(T.pool_backward(a, g), want)
    assert np.array_equal(T.pool(a), [[[[3, 2, 5, 7]]]]) and T.tied_positive_windows(a) == 3
    x = torch.from_numpy(a).requires_grad_()
    (F.max_pool2d(x, 2) * torch.from_numpy(g)).sum().backward()
    assert np.array_equal(x.grad.numpy(), want)


@pytest.mark.parametrize("name", T.IN_GOLDEN)
def test_restatement_equals_golden(name):
    g16 = golden("g16_trunk_grad.npz")
    r = T.flat(case(name)[1])
    keys = T.golden_keys(r)
    assert sorted(k.split("/", 1)[1] for k in g16.files if k.startswith(name + "/")) == sorted(keys)
    for key in keys:
        ref = g16["%s/%s" % (name, key)]
        assert ref.dtype in (np.int8, np.int32) and ref.shape == r[key].shape, (name, key)
        assert np.array_equal(ref.astype(np.float64), r[key]), (name, key)


def test_golden_is_small_and_below_2_to_24():
    g16 = golden("g16_trunk_grad.npz")
    assert os.path.getsize(T.GOLDEN) < 1000000
    assert 0 < float(g16["max_abs"]) < 2 ** 24
    assert sorted({f.split("/")[0] for f in g16.files if f != "max_abs"}) == sorted(T.IN_GOLDEN)


def test_float_cases_are_the_chain_of_float_blocks():
    c = T.make_float("f_b3_like")
    r = T.restate(c)
    assert r["y"].shape == T.y_shape(c["shape"]) and r["g_x"].shape == c["x"].shape and np.isfinite(r["g_x"]).all()
    assert K.rel_err(T.flat(T.restate(c, torch.float32))["g_x"], r["g_x"]) < 1e-4


def test_entry_points_in_library_header_and_ctypes_table():
    """pmp_trunk_saved_bytes needs neither a context nor a GPU."""
    from pmp_vvc_tip2023_amd import _lib
    header = open(os.path.join(ROOT, "include", "pmp.h")).read()
    lib = _lib.load()
    for name in NEW:
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
        assert re.search(r"^int(64_t)? %s\(" % name, header, re.M), name
    assert "#define PMP_TRUNK_MAX_BLOCKS 8" in header and _lib.PMP_TRUNK_MAX_BLOCKS == 8
    assert [f[0] for f in _lib.TrunkShape._fields_] == ["n", "h", "w", "cin", "nblocks", "cout", "k", "pool"]
    assert C.sizeof(_lib.TrunkShape) == 4 * (5 + 8 + 8 + 1)
    size = lambda shape: lib.pmp_trunk_saved_bytes(C.byref(_lib.trunk_shape(shape)))
    for name, shape in T.EXACT.items():
        n, h, w, cin, blocks, pool = shape
        pad = lambda ch: 16 if ch <= 16 else 32 if ch <= 32 else 64
        assert size(shape) == 4 * n * h * w * (pad(cin) + 2 * sum(pad(co) for co, _ in blocks)), name
    assert lib.pmp_trunk_saved_bytes(None) < 0
    n, h, w, cin, blocks, pool = T.EXACT["m1_like"]
    bad = [(0, h, w, cin, blocks, pool), (257, h, w, cin, blocks, pool), (n, 8, w, cin, blocks, pool), (n, 24, w, cin, blocks, pool),
           (n, h, 272, cin, blocks, pool), (n, h, w, 0, blocks, pool), (n, h, w, 65, blocks, pool), (n, h, w, cin, [], pool),
           (n, h, w, cin, [(64, 3)] * 9, pool), (n, h, w, cin, [(64, 5), (65, 3)], pool), (n, h, w, cin, [(0, 5), (64, 3)], pool),
           (n, h, w, cin, [(64, 4), (64, 3)], pool), (n, h, w, cin, [(64, 5), (64, 1)], pool), (n, h, w, cin, blocks, 2), (n, h, w, cin, blocks, -1)]
    for shape in bad:
        assert size(shape) == -1, shape
