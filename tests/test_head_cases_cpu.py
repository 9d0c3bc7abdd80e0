"""CPU: the head cases and their numpy float64 restatement (tests/head_cases.py) against the reference's own numbers
(tests/golden/g19_head_grad.npz, written by tools/gen_golden_head.py from nn.Conv2d, the in-place carry, F.interpolate and torch.cat
under autograd); the emulated orders of summation against the bounds; the gate's reference; the entry points in the library, the
header and the ctypes table; head.py's shape rule; the module's parameters against the oracle's weight dict; the size of the library."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT, golden
import head_cases as H

NEW = ("pmp_head_forward_device", "pmp_head_backward_device", "pmp_gate_forward_device", "pmp_gate_backward_device")
CSRC = os.path.join(ROOT, "pmp_vvc_tip2023_amd", "csrc")


@pytest.mark.parametrize("name", list(H.EXACT))
def test_exact_case_fits_float32_in_any_order(name):
    c = H.make_case(name)
    assert H.worst_partial_sum(c) < 2 ** 24
    for k in ("x", "w", "b", "prev", "q", "g_y", "g_att"):
        assert c[k] is None or (c[k].dtype == np.float32 and c[k].shape == H.sizes(c["shape"])[k] and np.array_equal(c[k], np.rint(c[k]))), k
    assert c["x"].min() == 0 and c["x"].max() == 15 and set(np.unique(c["w"])) <= {-1.0, 0.0, 1.0}
    assert (c["q"] is not None) == (c["g_att"] is not None) == (c["shape"][6] != 0)
    r = H.exact(name)[1]
    assert all(np.abs(r[k]).max() > 0 for k in ("y", "g_w", "g_b")) and (r["g_x"] is None) == (not c["want_g_x"])


def test_the_table_reaches_every_path():
    shapes = [H.EXACT[nm][0] for nm in H.EXACT]
    assert {s[3] for s in shapes} >= {1, 5, 8, 16} and {s[4] for s in shapes} == {1, 2}
    assert {s[5:] for s in shapes} == {(0, 0), (2, 1), (4, 2)}
    assert {(s[5:], H.EXACT[nm][1]) for nm, s in zip(H.EXACT, shapes)} >= {((0, 0), False), ((0, 0), True), ((2, 1), False), ((2, 1), True),
                                                                         ((4, 2), False), ((4, 2), True)}
    assert {H.EXACT[nm][2] for nm in H.EXACT} == {True, False} and {H.EXACT[nm][3] for nm in H.EXACT} == {True, False}
    assert (1, 8, 8) in {s[:3] for s in shapes} and {(16, 24), (24, 16), (256, 8)} <= {s[1:3] for s in shapes} and 3 in {s[0] for s in shapes}
    assert [H.head_np(H.EXACT[nm][0]) for nm in ("one_8x8", "two_items", "cap_255", "cap_256", "cap_258")] == \
        [(1, 1), (2, 1), (255, 128), (256, 128), (258, 128)]
    assert H.head_np((200, 16, 16, 8, 2, 2, 1)) == (800, 128)
    src = open(os.path.join(CSRC, "head_train.hip")).read()
    assert "HEAD_CAP = %d" % H.NP_CAP in src and "(items + 1) / 2 < HEAD_CAP ? (items + 1) / 2 : HEAD_CAP" in src


@pytest.mark.parametrize("name", H.IN_GOLDEN)
def test_restatement_equals_golden_bit_for_bit(name):
    g = golden("g19_head_grad.npz")
    c = H.make_case(name)
    want = H.restate(c)
    if c["prev"] is None:
        want["g_prev"] = None
    assert sorted(k.split("/")[1] for k in g.files if k.startswith(name + "/")) == sorted(k for k, v in want.items() if v is not None)
    for key, v in want.items():
        if v is not None:
            stored = g["%s/%s" % (name, key)]
            assert stored.shape == v.shape and H.same_bits(stored.astype(np.float32), H.as_f32(v)), (name, key)
            assert np.array_equal(stored.astype(np.float64), v), (name, key)


def test_golden_is_small_and_below_2_to_24():
    g = golden("g19_head_grad.npz")
    stem = os.path.join(os.path.dirname(H.GOLDEN), "g18_stem_grad.npz")
    assert os.path.getsize(H.GOLDEN) < os.path.getsize(stem) // 4 and float(g["max_abs"]) < 2 ** 24
    assert sorted({k.split("/")[0] for k in g.files if "/" in k}) == sorted(H.IN_GOLDEN)


def test_restatement_of_the_carry_gradient_includes_the_attention_windows():
    """g_prev[:, 0] is the gradient of the CARRIED y's channel 0: g_y alone only where there is no attention input."""
    c = H.make_case("b2_24x16")
    r = H.restate(c)
    assert not np.array_equal(r["g_prev"][:, 0], c["g_y"][:, 0]) and not r["g_prev"][:, 1:].any()
    assert np.array_equal(r["g_prev"][:, 0], c["g_y"][:, 0] + sum(H.windows(c["g_att"][:, 1].astype(np.float64), 2)))
    c3 = H.make_case("b3_16x16")
    assert np.array_equal(H.restate(c3)["g_prev"][:, 0], c3["g_y"][:, 0])


@pytest.mark.parametrize("name", list(H.FLOAT))
def test_emulated_order_stays_within_half_the_bound(name):
    c, ref, bound, A, emu = H.float_reference(name)
    kind = H.FLOAT[name][1]
    for key in H.BOUNDED:
        assert emu[key].dtype == np.float32 and emu[key].shape == ref[key].shape and np.isfinite(ref[key]).all()
        assert (bound[key] > 0).all(), (name, key)
        r = H.ratio(emu[key], ref[key], bound[key])
        print("%-14s %-4s emulated error = %.3f * 2^-24 * A" % (name, key, float((np.abs(emu[key].astype(np.float64) - ref[key]) / (H.EPS * A[key])).max())))
        assert r <= 0.5, (name, key, r)
    assert all(H.C_OF[k] == 2 * v for k, v in zip(H.BOUNDED, (H.C_Y_EMULATED, H.C_GX_EMULATED, H.C_GW_EMULATED, H.C_GB_EMULATED)))
    if kind == "positive":
        assert all((c[k] > 0).all() for k in ("x", "g_y", "g_att", "q"))
    if kind == "wide":
        nz = np.abs(c["x"][c["x"] != 0])
        assert (c["x"] == 0).any() and nz.min() >= 2.0 ** -20 and nz.max() <= 2.0 ** 8 and (c["x"] < 0).any()


@pytest.mark.parametrize("name", ["b2_24x16", "cap_258", "c16_att1"])
def test_emulation_is_exact_on_an_exact_case(name):
    c = H.make_case(name)
    got, want = H.emulate(c), H.restate(c)
    for key, v in want.items():
        assert (v is None) == (got[key] is None) and (v is None or H.same_bits(got[key], H.as_f32(v))), (name, key)


@pytest.mark.parametrize("name", list(H.ORDER))
def test_order_cases_tell_the_carry_behind_the_bias_from_the_carry_in_front(name):
    c = H.make_case(name, "order")
    x0, b, p0 = c["x"][:, 0], c["b"], c["prev"][:, 0]
    behind, in_front = (x0 + b[0]) + p0, (x0 + p0) + b[0]
    assert H.same_bits(H.emulate(c)["y"][:, 0], behind) and (behind != in_front).mean() > 0.1
    assert np.abs(H.emulate(c)["y"].astype(np.float64) - H.restate(c)["y"]).max() <= 2.0 ** -10


def test_gate_reference_rounds_product_and_sum_separately():
    c = H.gate_case(1023)
    r = H.gate_reference(c, True)
    fused = (c["g_acc"].astype(np.float64) + c["g_y"].astype(np.float64) * c["a"].astype(np.float64)).astype(np.float32)
    assert r["g_x"].dtype == np.float32 and (r["g_x"] != fused).any() and np.isfinite(r["g_x"]).all() and np.isfinite(r["y"]).all()
    for k in ("x", "a", "g_y", "g_acc"):
        bits = c[k].view(np.uint32)
        assert (bits == 0).any() and (bits == 0x80000000).any() and (((bits >> 23) & 0xFF == 0) & ((bits & 0x7FFFFF) != 0)).any(), k
    assert not np.array_equal(H.gate_reference(c, False)["g_x"], r["g_x"])


def test_shape_of_refuses_what_is_not_a_head():
    from pmp_vvc_tip2023_amd import head
    z = lambda *s: torch.zeros(s)
    assert head.shape_of(z(2, 8, 16, 24), z(2, 8, 3, 3), z(2), None, None, (0, 0)) == (2, 16, 24, 8, 2, 0, 0)
    assert head.shape_of(z(2, 8, 16, 24), z(2, 8, 3, 3), z(2), z(2, 2, 16, 24), z(2, 1, 8, 12), (4, 2)) == (2, 16, 24, 8, 2, 4, 2)
    assert head.shape_of(z(2, 8, 16, 24), z(1, 8, 3, 3), z(1), None, z(2, 1, 8, 12), (2, 1)) == (2, 16, 24, 8, 1, 2, 1)
    bad = [(z(2, 8, 16, 24), z(2, 8, 5, 5), z(2), None, None, (0, 0)), (z(2, 8, 16, 24), z(2, 4, 3, 3), z(2), None, None, (0, 0)),
           (z(2, 8, 16, 24), z(2, 8, 3, 3), None, None, None, (0, 0)), (z(2, 8, 16, 24), z(2, 8, 3, 3), z(3), None, None, (0, 0)),
           (z(8, 16, 24), z(2, 8, 3, 3), z(2), None, None, (0, 0)), (z(2, 8, 16, 24), z(2, 8, 3, 3), z(2), None, None, (2, 2)),
           (z(2, 8, 16, 24), z(2, 8, 3, 3), z(2), None, None, (2, 1)), (z(2, 8, 16, 24), z(2, 8, 3, 3), z(2), None, z(2, 1, 8, 12), (0, 0)),
           (z(2, 8, 16, 24), z(2, 8, 3, 3), z(2), None, z(2, 1, 16, 24), (2, 1)), (z(2, 8, 16, 24), z(2, 8, 3, 3), z(2), z(2, 1, 16, 24), None, (0, 0))]
    for args in bad:
        with pytest.raises(ValueError):
            head.shape_of(*args)


@pytest.mark.parametrize("luma", [True, False])
def test_module_state_dict_round_trips_with_the_oracle_weight_dict(luma):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import trained_like
    from pmp_vvc_tip2023_amd import msbd_net
    wts = trained_like.msbd_weights("Luma" if luma else "Chroma", 22 if luma else 27)
    net = msbd_net.MSBDNet(None, luma)
    sd = net.state_dict()
    assert list(sd) and sorted(sd) == sorted(wts) and len(list(net.parameters())) == 72
    assert all(tuple(sd[k].shape) == wts[k].shape for k in wts)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in wts.items()})
    assert all(np.array_equal(net.state_dict()[k].numpy(), wts[k]) for k in wts)


def test_entry_points_in_library_header_and_ctypes_table():
    from pmp_vvc_tip2023_amd import _lib, engine
    header = open(os.path.join(ROOT, "include", "pmp.h")).read()
    lib = _lib.load()
    for name in NEW:
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
        assert re.search(r"^int %s\(" % name, header, re.M), name
    assert "int n, h, w, cin, cout, up_q, up_y;" in header
    assert [f[0] for f in _lib.HeadShape._fields_] == ["n", "h", "w", "cin", "cout", "up_q", "up_y"] and C.sizeof(_lib.HeadShape) == 28
    s = _lib.head_shape((3, 24, 16, 8, 2, 4, 2))
    assert (s.n, s.h, s.w, s.cin, s.cout, s.up_q, s.up_y) == (3, 24, 16, 8, 2, 4, 2) and _lib.head_shape(s) is s
    assert [len(_lib.SIGNATURES[n][1]) for n in NEW] == [9, 11, 5, 8]
    for m in ("head_forward_device", "head_backward_device", "gate_forward_device", "gate_backward_device"):
        assert callable(getattr(engine.Engine, m))
    for src in ("Makefile", os.path.join("..", "..", "tools", "abl", "Makefile")):
        text = open(os.path.join(CSRC, src)).read()
        assert "head_train" in text and re.search(r"EXTRA_head_train = .*-ffp-contract=off", text), src
    main = open(os.path.join(CSRC, "train_check_main.cpp")).read()
    assert "head_shape_ok" in main and "head_att_refused" in main and "gate_count_ok" in main
