"""CPU: the QT tail's cases and their float64 restatement (tests/qtail_cases.py) against the golden (tests/golden/g20_qtail_grad.npz,
written by tools/gen_golden_qtail.py from nn.Conv2d, F.max_pool2d, F.interpolate and torch.cat under autograd); what the cases must
hold for the bit comparison to see the pools' tie rules; the entry points in the library, the header and the ctypes table;
pmp_qtail_saved_bytes without a GPU; qtail.py's shape rule and the module's parameters against the weight files; the host checks under
the sanitizers."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from conftest import ROOT, golden, golden_path
import qtail_cases as Q
import resblock_cases as K

NEW = ("pmp_qtail_saved_bytes", "pmp_qtail_forward_device", "pmp_qtail_backward_device", "pmp_qtail_unpack_device")
CSRC = os.path.join(ROOT, "pmp_vvc_tip2023_amd", "csrc")


@pytest.mark.parametrize("name", list(Q.EXACT))
def test_restatement_equals_golden_bit_for_bit(name):
    g = golden("g20_qtail_grad.npz")
    c, want = Q.exact(name)
    keys = Q.golden_keys(want)
    assert len(keys) == 13 and sorted(k.split("/")[1] for k in g.files if k.startswith(name + "/")) == sorted(keys)
    for key in keys:
        stored = g["%s/%s" % (name, key)]
        assert stored.dtype in (np.int8, np.int32) and stored.shape == want[key].shape, (name, key)
        assert np.array_equal(stored.astype(np.float64), want[key]) and K.same_bits(stored.astype(np.float32), K.as_f32(want[key])), (name, key)


def test_golden_is_small_and_records_the_largest_sum():
    g = golden("g20_qtail_grad.npz")
    assert os.path.getsize(golden_path("g20_qtail_grad.npz")) < 1000000
    worst = max(Q.worst_partial_sum(Q.exact(name)[0]) for name in Q.EXACT)
    assert float(g["max_abs"]) == worst and worst < 2 ** 24


@pytest.mark.parametrize("name", list(Q.EXACT))
def test_exact_case_holds_what_the_bit_comparison_needs(name):
    c, want = Q.exact(name)
    assert c["shape"] == Q.EXACT[name] and Q.worst_partial_sum(c) < 2 ** 24
    for a in [c["x4"], c["g_x9"]] + [t for blk in c["blocks"] for t in blk if t is not None]:
        assert a.dtype == np.float32 and np.array_equal(a, np.rint(a))
    # windows with tied positive maxima at every scale of the multi-scale pool and in q5's 2x2 pool
    for s in Q.SCALES:
        assert Q.tied_positive(want["s2"], s) > 0, s
    assert Q.tied_positive(want["s6"], 2) > 0
    # every gradient is there to be compared: g_x4 and the eleven weight gradients
    grads = [k for k in want if k.startswith("g_")]
    assert len(grads) == 12 and all(np.abs(want[k]).max() > 0 for k in grads + ["x9"])
    # the argmax of a hierarchy of 2x2 maxima would be seen
    assert not np.array_equal(Q.restate(c, hierarchical=True)["g_x4"], want["g_x4"])
    # float32 evaluates the restatement exactly
    r32 = Q.flat(Q.restate(c, torch.float32))
    assert all(r32[k].dtype == np.float32 and np.array_equal(r32[k].astype(np.float64), want[k]) for k in want)


def test_shapes_cover_the_nets_both_orientations_and_the_partitions():
    assert set(Q.EXACT.values()) == {(1, 16, 16), (3, 32, 16), (2, 16, 48), (5, 16, 16)}
    assert {(s, kind) for s, kind in Q.FLOAT.values()} == {((2, 16, 16), "randn"), ((2, 16, 16), "positive"), ((1, 32, 32), "randn"),
                                                           ((1, 32, 32), "positive")}
    assert all(Q.longest_wgrad_chain(s) <= 768 for s, _ in Q.FLOAT.values())
    c = Q.make_float("f_positive_16x16")
    assert c["x4"].min() > 0 and c["g_x9"].min() > 0 and c["x4"].dtype == np.float32


def test_multipool_rule_on_the_documented_tie():
    """A 4x4 window whose maxima sit at (0,3) and (1,0): row-major picks (0,3), the hierarchy of 2x2 maxima (1,0)."""
    x5 = np.zeros((1, 32, 16, 16))
    x5[0, 0, 0, 3] = x5[0, 0, 1, 0] = 5.0
    g6 = np.zeros((1, 128, 16, 16))
    g6[0, 64, 0:4, 0:4] = 1.0
    g = Q.multipool_backward(x5, g6)
    assert g[0, 0, 0, 3] == 16.0 and g[0, 0, 1, 0] == 0.0 and g.sum() == 16.0
    h = Q.multipool_backward(x5, g6, hierarchical=True)
    assert h[0, 0, 1, 0] == 16.0 and h[0, 0, 0, 3] == 0.0
    x6 = Q.multipool(x5)
    assert x6.shape == (1, 128, 16, 16) and (x6[0, 64, 0:4, 0:4] == 5.0).all() and x6[0, 64, 0, 4] == 0.0 and (x6[0, 96, 0:8, 0:8] == 5.0).all()
    assert x6[0, 32, 0, 2] == 5.0 and x6[0, 32, 0, 0] == 5.0 and x6[0, 32, 2, 0] == 0.0


def test_entry_points_in_library_header_and_ctypes_table():
    """pmp_qtail_saved_bytes needs neither a context nor a GPU."""
    from pmp_vvc_tip2023_amd import _lib, engine
    header = open(os.path.join(ROOT, "include", "pmp.h")).read()
    lib = _lib.load()
    for name in NEW:
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
        assert re.search(r"^int(64_t)? %s\(" % name, header, re.M), name
    assert [f[0] for f in _lib.QtailShape._fields_] == ["n", "h", "w"] and C.sizeof(_lib.QtailShape) == 12
    size = lambda shape: lib.pmp_qtail_saved_bytes(C.byref(_lib.qtail_shape(shape)))
    for n, h, w in list(Q.EXACT.values()) + [(200, 16, 16), (256, 256, 256), (1, 32, 32)]:
        h2, w2 = (h // 2 + 15) // 16 * 16, (w // 2 + 15) // 16 * 16
        assert size((n, h, w)) == 4 * n * (h * w * (64 + 6 * 32) + h2 * w2 * 2 * 16) > 0, (n, h, w)
    assert size((200, 16, 16)) == 58982400 and "58 982 400" in header
    assert engine.Engine.qtail_saved_bytes((1, 16, 16)) == size((1, 16, 16))
    assert lib.pmp_qtail_saved_bytes(None) == -1
    for shape in [(0, 16, 16), (257, 16, 16), (1, 8, 16), (1, 24, 16), (1, 272, 16), (1, 16, 0)]:
        assert size(shape) == -1, shape
        with pytest.raises(_lib.PmpError):
            engine.Engine.qtail_saved_bytes(shape)


def test_train_check_passes_with_the_tail_matrix():
    """train_check.h with a main of its own under AddressSanitizer and UBSan: a stand-alone CPU program, built and run once."""
    r = subprocess.run(["make", "-s", "-C", CSRC, "traincheck"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "train_check: ok" in r.stdout, (r.stdout + r.stderr)[-2000:]
    assert "qtail_shape_ok" in open(os.path.join(CSRC, "train_check_main.cpp")).read()


def test_qtail_shape_rule():
    from pmp_vvc_tip2023_amd import qtail
    c = Q.make_exact("nets")
    t = lambda a: None if a is None else torch.from_numpy(a)
    blocks = [tuple(t(a) for a in blk) for blk in c["blocks"]]
    assert qtail.shape_of(t(c["x4"]), blocks) == (1, 16, 16)
    four_d = [(w0, w2, None if wsc is None else wsc.reshape(wsc.shape + (1, 1))) for w0, w2, wsc in blocks]
    assert qtail.shape_of(t(c["x4"]), four_d) == (1, 16, 16)
    bad = [(t(c["x4"])[:, :63], blocks), (t(c["x4"])[0], blocks), (t(c["x4"]), blocks[:3]), (t(c["x4"]), blocks + blocks[:1]),
           (t(c["x4"]), [blocks[0], blocks[1], (blocks[2][0], blocks[2][1], blocks[0][2]), blocks[3]]),
           (t(c["x4"]), [blocks[0], (blocks[1][0], blocks[1][1], None), blocks[2], blocks[3]]),
           (t(c["x4"]), [blocks[0], blocks[0], blocks[2], blocks[3]]),
           (t(c["x4"]), [blocks[0], blocks[1], blocks[2], (torch.zeros(8, 32, 5, 5), blocks[3][1], blocks[3][2])])]
    for x4, bl in bad:
        with pytest.raises(ValueError):
            qtail.shape_of(x4, bl)


@pytest.mark.parametrize("comp, qp", [("Luma", 22), ("Chroma", 27)])
def test_qnet_parameters_are_the_weight_files(comp, qp):
    """QNet has the reference's 20 tensors under its names, and a state_dict round trip with the weight dict is bit for bit."""
    from pmp_vvc_tip2023_amd import q_net, weights as W
    wq, _ = W.load_net_weights(comp + "_Q", qp)
    net = q_net.QNet(None, luma=comp == "Luma")
    sd = net.state_dict()
    assert len(sd) == 20 and sorted(sd) == sorted(wq)
    names = ["conv_q1.weight", "conv_q1.bias", "conv_q2.weight", "conv_q2.bias"]
    for i in range(1, 7):
        names += ["resblock_q%d.left.0.weight" % i, "resblock_q%d.left.2.weight" % i] + (["resblock_q%d.shortcut.0.weight" % i] if i != 2 and i != 5 else [])
    assert sorted(names) == sorted(sd)
    net.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in wq.items()})
    for k, v in net.state_dict().items():
        assert tuple(v.shape) == tuple(np.asarray(wq[k]).shape) and K.same_bits(v.numpy(), np.asarray(wq[k], np.float32)), k
