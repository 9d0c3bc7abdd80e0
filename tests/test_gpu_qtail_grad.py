"""GPU: a QT net's tail as one call, forward and backward (include/pmp.h: pmp_qtail_*; csrc/api_train.cpp, qtail_train.hip;
pmp_vvc_tip2023_amd/qtail.py).

Bounds.  On the EXACT cases of tests/qtail_cases.py every value is an integer and every partial sum stays below 2^24: x9, g_x4 and the
eleven weight gradients must equal the golden (torch autograd in float64) BIT FOR BIT, and the nine saved tensors the restatement the
golden was checked against, in poisoned workspaces, into NaN-filled outputs and a 0xFF-filled d_saved.  On float values every
operation is held to grad_cases' bound, locally (qtail_cases' docstring), with C_CONV for what conv_mfma makes and C_WGRAD for what
wgrad_partial_kernel makes; the multi-scale pool's backward, additions only, is pinned bit for bit.
Largest |gpu - ref64| / bound measured on an MI355X over the four float cases (`pytest -s` prints them per tensor):
    t / out (conv_mfma) 0.301 (q3's t, f_positive_32x32)    weight gradients 0.336 (q6's g_w2, f_positive_32x32)    g_x4 below 0.001
The gradients far from g_x9 (q3's, q4's, g_x4) sit at a few thousandths of their bounds and less: P, the error an upstream gradient
may carry, is pushed through four blocks' absolute-value companions and dominates there.  What holds those tensors tightly is the
exact cases.
"""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import grad_cases as G
import qtail_cases as Q
import resblock_cases as K
import train_rig as R
import trunk_cases as T
from cases_common import ratio

pytestmark = pytest.mark.gpu

P, up, nan, num, check_bits = R.P, R.up, R.nan, R.num, R.check_bits
eng = R.engine_fixture(poison=1)
Dev, run = R.TailDev, R.TailDev.run


@functools.lru_cache(maxsize=None)
def exact(name):
    """-> (case, what a kernel must produce: the golden's outputs and the restatement's saved tensors, float32); computed once."""
    c, r = Q.exact(name)
    want = {k: K.as_f32(v) for k, v in r.items()}
    with np.load(Q.GOLDEN) as z:
        for k in Q.golden_keys(r):
            gold = z["%s/%s" % (name, k)]
            assert np.array_equal(gold, r[k]), (name, k)
            want[k] = K.as_f32(gold)
    return c, want


_FLOAT = {}


def float_results(e, name):
    """A float case and its results on the GPU, computed once and shared (the fixture's engine is the module's only one)."""
    if name not in _FLOAT:
        c = Q.make_float(name)
        _FLOAT[name] = (c, run(e, c))
    return _FLOAT[name]


# ---- 1. every exact case equals the golden, in poisoned workspaces, into NaN-filled outputs and a 0xFF-filled d_saved
@pytest.mark.parametrize("name", list(Q.EXACT))
def test_exact_cases_bit_equal(eng, name):
    c, want = exact(name)
    got = run(eng, c)
    assert sorted(got) == sorted(want) and len([k for k in want if k.startswith("g_w")]) == 11
    check_bits(name, got, want)
    assert K.same_bits(got["s0"], c["x4"]) and K.same_bits(got["s8"], got["x9"])


def test_without_g_x4(eng):
    c, want = exact("wide")
    got = run(eng, c, want_g_x=False)
    assert np.isnan(got["g_x4"]).all()
    check_bits("no g_x4", got, want, skip=("g_x4",))


# ---- 2. q3 and q5 are pmp_resblock_forward_device's block, bit for bit, on float values
def test_q3_and_q5_equal_the_block_call(eng):
    c, got = float_results(eng, "f_randn_16x16")
    n, h, w = c["shape"]
    for blk, (i_x, i_t, i_o), (ci, co) in ((0, (0, 1, 2), (64, 32)), (2, (4, 5, 6), (32, 32))):
        x, (w0, w2, wsc) = up(got["s%d" % i_x]), [up(a) for a in c["blocks"][blk]]
        t, out = nan(n, co, h, w), nan(n, co, h, w)
        R.torch_done()
        eng.resblock_forward_device((n, h, w, ci, co, 3), P(x), P(w0), P(w2), P(wsc), P(t), P(out))
        eng.synchronize()
        assert np.abs(num(out)).max() > 0
        assert K.same_bits(num(t), got["s%d" % i_t]) and K.same_bits(num(out), got["s%d" % i_o]), blk


# ---- 3. float values: every operation within grad_cases' bound of float64 on the inputs, masks and maxima the GPU saved
def _d(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, np.float64))


C_POOL = 66          # the multi-scale pool's backward: at most 63 + 3 float32 additions per element, each within 2^-24 of a partial sum <= A


def local_block(x, t, out, blk, g, b_g):
    """One block on the GPU's own x, t, out (float32 values as float64), upstream gradient g with the bound b_g it carries ->
    ({name: (ref, bound)} for t, out, g_w0, g_w2, g_wsc, g_x), all float64 torch tensors."""
    w0, w2 = _d(blk[0]), _d(blk[1])
    wsc4 = None if blk[2] is None else _d(blk[2]).reshape(blk[2].shape[0], blk[2].shape[1], 1, 1)
    conv = lambda a, wt, pp=1: F.conv2d(a, wt, padding=pp)
    convt = lambda a, wt, pp=1: F.conv_transpose2d(a, wt, padding=pp)
    wg = lambda a, wt, gg, pp=1: torch.nn.grad.conv2d_weight(a, wt.shape, gg, padding=pp)
    rnd = lambda c_, A, ref, PP=0.0: c_ * G.EPS * A + G.R_STORE * ref.abs() + PP
    zero = torch.zeros((), dtype=torch.float64)
    r = {}
    t_ref = F.relu(conv(x, w0))
    r["t"] = (t_ref, rnd(G.C_CONV, conv(x.abs(), w0.abs()), t_ref))
    sc, asc = (x, x.abs()) if wsc4 is None else (conv(x, wsc4, 0), conv(x.abs(), wsc4.abs(), 0))
    o_ref = F.relu(conv(t, w2) + sc)
    r["out"] = (o_ref, rnd(G.C_CONV, conv(t, w2.abs()) + asc, o_ref))
    gu, b_gu = torch.where(out > 0, g, zero), torch.where(out > 0, b_g, zero)
    ref = wg(t, w2, gu)
    r["g_w2"] = (ref, rnd(G.C_WGRAD, wg(t, w2, gu.abs()), ref, wg(t, w2, b_gu)))
    if wsc4 is not None:
        ref = wg(x, wsc4, gu, 0)
        r["g_wsc"] = (ref.reshape(blk[2].shape), rnd(G.C_WGRAD, wg(x.abs(), wsc4, gu.abs(), 0), ref, wg(x.abs(), wsc4, b_gu, 0)).reshape(blk[2].shape))
    m = t > 0
    gt = torch.where(m, convt(gu, w2), zero)
    b_gt = torch.where(m, rnd(G.C_CONV, convt(gu.abs(), w2.abs()), gt, convt(b_gu, w2.abs())), zero)
    ref = wg(x, w0, gt)
    r["g_w0"] = (ref, rnd(G.C_WGRAD, wg(x.abs(), w0, gt.abs()), ref, wg(x.abs(), w0, b_gt)))
    a_gx = convt(gt.abs(), w0.abs()) + (gu.abs() if wsc4 is None else convt(gu.abs(), wsc4.abs(), 0))
    p_gx = convt(b_gt, w0.abs()) + (b_gu if wsc4 is None else convt(b_gu, wsc4.abs(), 0))
    ref = convt(gt, w0) + (gu if wsc4 is None else convt(gu, wsc4, 0))
    r["g_x"] = (ref, rnd(G.C_CONV, a_gx, ref, p_gx))
    return r


@pytest.mark.parametrize("name", list(Q.FLOAT))
def test_float_cases_within_the_bound(eng, name):
    c, got = float_results(eng, name)
    assert Q.longest_wgrad_chain(c["shape"]) <= 768
    s = [got["s%d" % i].astype(np.float64) for i in range(9)]
    assert K.same_bits(got["s0"], c["x4"]) and K.same_bits(got["s8"], got["x9"])
    x6, x8 = Q.multipool(s[2]), T.pool(s[6])
    ins, ts, outs = [s[0], x6, s[4], x8], [s[1], s[3], s[5], s[7]], [s[2], s[4], s[6], s[8]]
    g, b_g = _d(c["g_x9"]), torch.zeros(c["g_x9"].shape, dtype=torch.float64)
    worst = {}
    for i in (3, 2, 1, 0):
        r = local_block(_d(ins[i]), _d(ts[i]), _d(outs[i]), c["blocks"][i], g, b_g)
        checks = [("t", got["s%d" % (2 * i + 1)]), ("out", got["s%d" % (2 * i + 2)])] + \
                 [(k, got["%s_%d" % (k, i)]) for k in ("g_w0", "g_w2", "g_wsc") if k in r] + ([("g_x", got["g_x4"])] if i == 0 else [])
        for k, have in checks:
            ref, bnd = (v.numpy() for v in r[k])
            assert np.isfinite(have).all() and np.abs(ref).max() > 0, (name, i, k)
            worst["q%d %s" % (i + 3, k)] = q = ratio(have, ref, bnd)
            print("%s q%d %-5s |gpu - ref64| / bound = %.3f" % (name, i + 3, k, q))
        g, b_g = (v.numpy() for v in r["g_x"])
        if i == 3:
            g, b_g = T.pool_backward(s[6], g), T.pool_backward(s[6], b_g)
        if i == 1:
            a = Q.multipool_backward(s[2], np.abs(g))
            g, b_g = Q.multipool_backward(s[2], g), Q.multipool_backward(s[2], b_g) + C_POOL * G.EPS * a
        g, b_g = _d(g), _d(b_g)
    assert max(worst.values()) <= 1.0, {k: v for k, v in worst.items() if v > 1.0}


# ---- 4. the multi-scale pool's backward, additions only, bit for bit: selection weights make everything around it exact
def selection_case(name):
    """The float case's x4 and g_x9 with weights that only select and scale by powers of two: w0 = w2 = 0 everywhere, every shortcut
    one-hot per INPUT channel.  Backward every data gradient is then a single exact product per element, except the window sums of
    the multi-scale pool, and g_x4[:, 0:32] is +-q3's upstream gradient: g_x5 where x5 > 0."""
    c = Q.make_float(name)
    z = lambda a: np.zeros_like(a)
    onehot = lambda co, ci, val: np.stack([np.where(np.arange(co) == j % co, val(j), 0.0) for j in range(ci)], axis=1).astype(np.float32)
    b = c["blocks"]
    c["blocks"] = [(z(b[0][0]), z(b[0][1]), onehot(32, 64, lambda j: 1.0 if j < 32 else -1.0)),
                   (z(b[1][0]), z(b[1][1]), onehot(32, 128, lambda j: 2.0 ** -(j // 32))),
                   (z(b[2][0]), z(b[2][1]), None),
                   (z(b[3][0]), z(b[3][1]), onehot(8, 32, lambda j: 1.0))]
    return c


@pytest.mark.parametrize("name", list(Q.FLOAT))
def test_multiscale_pool_backward_bits(eng, name):
    c = selection_case(name)
    got = run(eng, c)
    s = [got["s%d" % i] for i in range(9)]
    f = np.float32
    zero = f(0)
    gu6 = np.where(s[8] > 0, c["g_x9"], zero)
    g_x8 = np.concatenate([gu6] * 4, axis=1)                                   # input channel j reads output j % 8
    gu5 = np.where(s[6] > 0, T.pool_backward(s[6], g_x8), zero)               # q5: w0 = 0, so g_x7 = gu5
    gu4 = np.where(s[4] > 0, gu5, zero)
    g6 = np.concatenate([gu4 * f(2.0 ** -k) for k in range(4)], axis=1)
    assert g6.dtype == np.float32
    g_x5 = Q.multipool_backward(s[2], g6)
    assert g_x5.dtype == np.float32
    gu3 = np.where(s[2] > 0, g_x5, zero) + zero
    assert np.count_nonzero(gu3) > gu3.size // 8
    # the order matters on these values: the window sums added in float64 and rounded once give other bits somewhere
    once = np.where(s[2] > 0, Q.multipool_backward(s[2], g6.astype(np.float64)).astype(f), zero) + zero
    assert not K.same_bits(once, gu3)
    assert K.same_bits(got["g_x4"][:, 0:32], gu3), np.argwhere(got["g_x4"][:, 0:32] != gu3)[:4]
    assert K.same_bits(got["g_x4"][:, 32:64], -gu3 + zero)


# ---- 5. determinism: twice, on a second stream, on a second context
def test_same_bits_on_every_run_stream_and_context(eng):
    R.same_bits_on_every_run_stream_and_context(eng, run, Q.make_case((3, 32, 16), 77, "randn"), nonzero=True)


# ---- 6. refusals: PMP_E_INVALID before any launch, nothing written
def test_refusals_write_nothing(eng):
    c = exact("nets")[0]
    d = Dev(eng, c)                                                    # never run: everything it owns must stay as filled
    ok = Dev(eng, c)                                                   # a finished forward, for the calls that read d_saved
    ok.forward(eng)
    eng.synchronize()
    saved_ok = ok.saved.clone()
    dense = nan(*ok.x.shape)
    other, other_g = up(c["blocks"][0][2]), nan(*c["blocks"][0][2].shape)
    call = R.chain_refusal_call(eng, Dev, lambda nm, what: d if what == "forward" else ok, dense)

    bad_shapes = [(0, 16, 16), (257, 16, 16), (1, 8, 16), (1, 24, 16), (1, 272, 16), (1, 16, 0), (1, 16, 40)]
    tries = []
    for what in ("forward", "backward", "unpack"):
        tries += [("shape %s" % (s,), "nets", what, dict(shape=s)) for s in bad_shapes]
        tries += [("null shape", "nets", what, dict(null_shape=True)), ("null d_saved", "nets", what, dict(saved=None)),
                  ("d_saved at +4 bytes", "nets", what, dict(saved=P(ok.saved if what != "forward" else d.saved) + 4))]
    for what in ("forward", "backward"):
        tries += [("null d_w", "nets", what, dict(null_w=True)), ("null w0 of q3", "nets", what, dict(w={0: None}, g_w={0: None})),
                  ("null w2 of q6", "nets", what, dict(w={10: None}, g_w={10: None})),
                  ("q5 with a wsc", "nets", what, dict(w={8: P(other)}, g_w={8: P(other_g)})),
                  ("q4 without its wsc", "nets", what, dict(w={5: None}, g_w={5: None})),
                  ("misaligned w0", "nets", what, dict(w={0: P(d.w[0]) + 2}))]
    tries += [("null x4", "nets", "forward", dict(x4=None)), ("null x9", "nets", "forward", dict(x9=None)),
              ("x9 overlaps x4", "nets", "forward", dict(x9=P(d.x) + 64)), ("x9 inside d_saved", "nets", "forward", dict(x9=P(d.saved) + 256)),
              ("d_saved is x4", "nets", "forward", dict(saved=P(d.x))), ("misaligned x4", "nets", "forward", dict(x4=P(d.x) + 2)),
              ("null g_x9", "nets", "backward", dict(g_x9=None)), ("null d_g_w", "nets", "backward", dict(null_g_w=True)),
              ("null g_w0 of q4", "nets", "backward", dict(g_w={3: None})), ("a g_wsc for q5", "nets", "backward", dict(g_w={8: P(other_g)})),
              ("no g_wsc for q4", "nets", "backward", dict(g_w={5: None})),
              ("g_x4 over g_x9", "nets", "backward", dict(g_x4=P(ok.g_y))), ("g_x4 inside d_saved", "nets", "backward", dict(g_x4=P(ok.saved) + 1024)),
              ("g_w0 is g_w2", "nets", "backward", dict(g_w={6: P(ok.g_w[7])})), ("misaligned g_x9", "nets", "backward", dict(g_x9=P(ok.g_y) + 2)),
              ("null dense", "nets", "unpack", dict(dense=None)), ("index -1", "nets", "unpack", dict(index=-1)),
              ("index 9", "nets", "unpack", dict(index=9)), ("dense inside d_saved", "nets", "unpack", dict(dense=P(ok.saved) + 512)),
              ("misaligned dense", "nets", "unpack", dict(dense=P(dense) + 2))]
    R.refuse_all(eng, tries, call)
    R.check_untouched("never run", d.outputs(), d.inputs(c))
    R.check_untouched("ok", ok.outputs(), ok.inputs(c), skip=("x9", "d_saved"))                 # its forward ran
    assert torch.isnan(dense).all() and torch.isnan(other_g).all() and torch.equal(ok.saved, saved_ok)
    # and the calls after a refusal still work
    ok.backward(eng)
    check_bits("after the refusals", ok.results(eng), exact("nets")[1])


# ---- 7. under torch.autograd: qtail_of on a net's modules, and what is not a tail
def test_qtail_of_modules_and_value_errors(eng):
    from pmp_vvc_tip2023_amd import qtail
    c, want = exact("five")
    net = torch.nn.Module()
    for i, blk in enumerate(c["blocks"]):
        setattr(net, "resblock_q%d" % (i + 3), R.reference_block(*blk))
    net.cuda()
    try:
        x4 = up(c["x4"]).requires_grad_()
        x9 = qtail.qtail_of(eng, net, x4)
        x9.backward(up(c["g_x9"]))
        frozen = qtail.qtail_of(eng, net, x4.detach())
        torch.cuda.synchronize()
        assert frozen.requires_grad and K.same_bits(num(frozen.detach()), want["x9"])
        with pytest.raises(ValueError):
            qtail.qtail(eng, x4[:, :32], [tuple(up(a) for a in blk) for blk in c["blocks"]])
        with pytest.raises(ValueError):
            qtail.qtail(eng, x4, [tuple(None if a is None else up(a) for a in blk) for blk in c["blocks"][:3]])
        with pytest.raises(ValueError):
            qtail.qtail(eng, x4, [tuple(None if a is None else up(a) for a in c["blocks"][i]) for i in (0, 1, 3, 3)])
    finally:
        eng.set_stream(0)
    got = {"x9": num(x9.detach()), "g_x4": num(x4.grad)}
    for i in range(4):
        m = getattr(net, "resblock_q%d" % (i + 3))
        got["g_w0_%d" % i], got["g_w2_%d" % i] = num(m.left[0].weight.grad), num(m.left[2].weight.grad)
        if len(m.shortcut):
            got["g_wsc_%d" % i] = num(m.shortcut[0].weight.grad).reshape(want["g_wsc_%d" % i].shape)
    assert sorted(got) == sorted(Q.golden_keys(want))
    check_bits("qtail_of", got, {k: want[k] for k in got})
