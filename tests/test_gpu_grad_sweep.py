"""GPU: the ResidualBlock and trunk gradients over the shapes include/pmp.h accepts - the table of tests/grad_cases.py, whose reach
tests/test_grad_cases_cpu.py asserts: every wgrad_partial_kernel<K,NCO> at every number of input groups, ragged channel counts, n = 1
and 256, maps up to 256 x 256, the edges of the reduction's partition, eight blocks, masks on the edge of `> 0`, subnormals, caller
tensors that are 4-byte but not 16-byte aligned.

Bounds.  EXACT cases (integers below 2^24, or exact subnormals): every output equals the float64 restatement BIT FOR BIT, no element
left out, into NaN-filled buffers in workspaces poisoned with pattern 2.  FLOAT cases: every element within grad_cases' per-element
bound, |gpu - ref64| <= c * 2^-24 * A + 2^-23 * |ref64| + P; `pytest -s` prints the largest ratio per kernel class, recorded in
grad_cases' docstring.  Float trunks equal the chain of pmp_resblock_*_device calls bit for bit."""
import numpy as np
import pytest

import grad_cases as G
import resblock_cases as K
import train_rig as R

pytestmark = pytest.mark.gpu

GRADS, Off4 = R.GRADS, R.Off4
NGROUPS = G.NGROUPS
WORST = {}                 # kernel class -> (largest ratio, case): printed as it grows
eng = R.engine_fixture(poison=2)


def block_exact(name):
    """-> (case with t and out as float32, the float64 restatement as the float32 a kernel must produce)."""
    c = G.make_block(name)
    want = {k: K.as_f32(v) for k, v in K.restate(c).items()}
    c["t"], c["out"] = want["t"], want["out"]
    return c, want


# ---- 1. every exact block case, forward and backward
@pytest.mark.parametrize("group", range(NGROUPS))
def test_exact_block_cases_bit_equal(eng, group):
    names = list(G.BLOCKS)[group::NGROUPS]
    assert names
    for name in names:
        c, want = block_exact(name)
        R.check_bits(name + " forward", R.dev_forward(eng, c), want, ("t", "out"))
        R.check_bits(name + " backward", R.dev_backward(eng, c), want, GRADS)


# ---- 2. masks on the edge of `> 0`, and subnormal results
@pytest.mark.parametrize("name", list(G.MASK_EDGES))
def test_mask_edges_bit_equal(eng, name):
    c = G.make_block(name)
    want = {k: K.as_f32(v) for k, v in G.mask_edges_reference(c)[0].items()}
    assert np.abs(want["g_w2"]).max() < 2.0 ** -126 and (want["g_w2"] != 0).mean() > 0.9
    R.check_bits(name, R.dev_backward(eng, c), want, GRADS)


def test_subnormal_trunk_bit_equal(eng):
    base, flat = G.trunk_exact(G.SUBNORMAL_TRUNK)
    c = G.scaled_trunk(base)
    want = {k: K.as_f32(v) for k, v in G.scaled_restatement(flat).items()}
    got = R.run_trunk(eng, c)
    assert sorted(k for k in got if k != "x") == sorted(want)
    R.check_bits("subnormal trunk", got, want)
    assert K.same_bits(got["x"], c["x"]) and np.abs(got["y"]).max() > 0


# ---- 3. float values: every element within its bound
def _classes(shape):
    n, h, w, cin, cout, k = shape
    cls = {"t": "conv %dx%d" % (k, k), "out": "conv %dx%d + shortcut" % (k, k), "g_x": "data gradient %dx%d" % (k, k)}
    cls.update({out: "wgrad_partial_kernel<%d,%d>" % (kk, nco) for out, kk, nco, _, _, _ in G.wgrads(shape)})
    return cls


@pytest.mark.parametrize("name", list(G.FLOAT))
def test_float_case_within_its_bound_per_element(eng, name):
    c = G.make_block(*G.FLOAT[name])
    t32, out32, ref, bnd, _ = G.float_reference(c)
    c["t"], c["out"] = t32, out32
    got = R.run_block(eng, c)
    cls = _classes(c["shape"])
    ratios = {}
    for key in K.OUTPUTS:
        if ref[key] is None:
            continue
        assert got[key].shape == ref[key].shape and np.isfinite(got[key]).all(), (name, key)
        ratios[key] = G.ratio(got[key], ref[key], bnd[key])
        if ratios[key] > WORST.get(cls[key], (0.0, ""))[0]:
            WORST[cls[key]] = (ratios[key], name)
    print("%s: |gpu - ref64| / bound  %s" % (name, "  ".join("%s %.3f" % kv for kv in ratios.items())))
    print("largest so far: " + "; ".join("%s %.3f (%s)" % (k, v[0], v[1]) for k, v in sorted(WORST.items())))
    for key, r in ratios.items():
        assert r <= 1.0, (name, key, r)


# ---- 4. every trunk case; float twins against the chain of block calls
@pytest.mark.parametrize("name", list(G.TRUNKS))
def test_exact_trunk_cases_bit_equal(eng, name):
    c, flat = G.trunk_exact(name)
    want = {k: K.as_f32(v) for k, v in flat.items()}
    got = R.run_trunk(eng, c)
    assert sorted(k for k in got if k != "x") == sorted(want)
    R.check_bits(name, got, want)
    assert K.same_bits(got["x"], c["x"]), "unpack of x"


@pytest.mark.parametrize("name", G.TRUNK_FLOAT)
def test_float_trunk_equals_chain_of_block_calls(eng, name):
    c = G.make_trunk(name, "float")
    d = R.TrunkDev(eng, c)
    d.forward(eng)
    d.backward(eng)
    ts, outs = d.unpack(eng)
    eng.synchronize()
    got = d.results(eng, ts, outs)
    want = R.chain(eng, c, ts, outs)
    assert sorted(k for k in got if k != "x") == sorted(want)
    for k, v in want.items():
        assert np.isfinite(v).all() and np.abs(v).max() > 0, (name, k)
    R.check_bits(name, got, want)


# ---- 5. caller tensors that are 4-byte but not 16-byte aligned
@pytest.mark.parametrize("name", ["r_k5_1to17", "p_k3_64to64", "r_k3_31to17"])
def test_block_on_tensors_4_bytes_off(eng, name):
    if name == "r_k3_31to17":                                                # one on float values: the same bits, not only the same integers
        c = G.make_block(name, "randn")
        c["t"], c["out"] = (K.as_f32(v) for v in K.forward(c["x"], c["w0"], c["w2"], c["wsc"]))
    else:
        c, _ = block_exact(name)
    want = R.run_block(eng, c)                                               # the aligned run
    sc = c["wsc"] is not None
    d = {k: Off4(R.up(c[k])) for k in R.BWD_IN if c[k] is not None}
    o = {k: Off4(v) for k, v in R.nan_dev(c, [k for k in ("t", "out") + GRADS if sc or k != "g_wsc"]).items()}
    p = lambda m, k: m[k].view.data_ptr() if k in m else None
    R.torch_done()
    eng.resblock_forward_device(c["shape"], *[p(d, k) for k in R.FWD_IN], p(o, "t"), p(o, "out"))
    eng.resblock_backward_device(c["shape"], *[p(d, k) for k in R.BWD_IN], *[p(o, k) for k in GRADS])
    eng.synchronize()
    for k, v in o.items():
        got = v.view.cpu().numpy()
        assert not np.isnan(got).any() and K.same_bits(got, want[k]), (name, k)
        assert v.guards_intact(), (name, k, "written outside the tensor")
    for k, v in d.items():
        assert v.guards_intact() and K.same_bits(v.view.cpu().numpy(), c[k]), (name, k, "an input changed")


@pytest.mark.parametrize("name", ["wide_pool63", "mixed5"])
def test_trunk_on_tensors_4_bytes_off(eng, name):
    c, _ = G.trunk_exact(name)
    want = R.run_trunk(eng, c)                                                    # the aligned run
    d = R.TrunkDev(eng, c)
    held = []

    def off(t):
        if t is None:
            return None
        held.append(Off4(t))
        return held[-1].view

    d.x, d.g_y, d.y, d.g_x = off(d.x), off(d.g_y), off(d.y), off(d.g_x)
    d.w, d.g_w = [off(a) for a in d.w], [off(a) for a in d.g_w]
    assert d.saved.data_ptr() % 16 == 0                                      # d_saved keeps its 16 bytes
    R.torch_done()
    d.forward(eng)
    d.backward(eng)
    n, h, w = d.shape[:3]
    ts, outs = [], []
    for i, (cout, _) in enumerate(d.shape[4]):                               # unpack into tensors 4 bytes off, too
        ts.append(off(R.nan(n, cout, h, w)))
        outs.append(off(R.nan(n, cout, h, w)))
        R.torch_done()
        eng.trunk_unpack_device(d.shape, R.P(d.saved), 2 * i + 1, R.P(ts[-1]))
        eng.trunk_unpack_device(d.shape, R.P(d.saved), 2 * i + 2, R.P(outs[-1]))
    got = d.results(eng, ts, outs)
    assert sorted(got) == sorted(want)
    for k, v in want.items():
        assert not np.isnan(v).any() and K.same_bits(got[k], v), (name, k)
    assert all(a.guards_intact() for a in held), "written outside a tensor"
