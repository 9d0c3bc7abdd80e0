"""GPU: the nets' first layers, forward and backward (include/pmp.h: pmp_stem_*; csrc/api_train.cpp, stem_train.hip;
pmp_vvc_tip2023_amd/stem.py).

Bounds.  On the EXACT cases of tests/stem_cases.py every value is an integer and every partial sum is below 2^24: float32 arithmetic is
exact in any order, and y, g_x and every weight and bias gradient must equal the float64 restatement BIT FOR BIT, no element left out,
in poisoned workspaces, into NaN-filled outputs, with x an interior view of a larger NaN-filled allocation (a read beyond x shows as
NaN, and x is only 4-byte aligned).  On the FLOAT cases every element must stay within stem_cases' bound
    |gpu - ref64| <= c * 2^-24 * A + 2^-23 * |ref64|,   c = 14 (forward), 25 (weight and bias gradient), 15.4 (input gradient),
twice what the emulated order of additions reaches; the backward pass is given the float32 rounding of the float64 forward, so the
mask is the reference's.  Largest ratios measured on an MI355X: stem_cases' docstring."""
import copy
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import stem_cases as S
import train_rig as R

pytestmark = pytest.mark.gpu
RATIOS = {}
P, nan, check_bits = R.P, R.nan, R.check_bits_same_keys
Dev, run = R.StemDev, R.run_stem
eng = R.engine_fixture()


# ---- 1. every exact case equals the restatement, in poisoned workspaces, into NaN-filled outputs; without g_x its buffer stays NaN
@pytest.mark.parametrize("name", list(S.EXACT))
def test_exact_cases_bit_equal(eng, name):
    c, want = S.exact(name)
    try:
        for pattern in (1, 2):
            eng._ck(eng.lib.pmp_debug_poison_workspace(eng.h, pattern))
            check_bits("poison %d" % pattern, run(eng, c), want)
        got = run(eng, c, want_g_x=False)
        assert np.isnan(got["g_x"]).all()
        check_bits("no g_x", got, want, skip=("g_x",))
    finally:
        eng._ck(eng.lib.pmp_debug_poison_workspace(eng.h, 0))


# ---- 2. determinism: twice, on a second stream, on a second context
def test_same_bits_on_every_run_stream_and_context(eng):
    R.same_bits_on_every_run_stream_and_context(eng, run, S.make_case("f_luma", "randn"), nonzero=True)


# ---- 3. float values within the bound, every element
@pytest.mark.parametrize("name", list(S.FLOAT))
def test_float_cases_within_the_bound(eng, name):
    c, y32, ref, bound, A = S.float_reference(name)
    d = Dev(c)
    d.forward(eng)
    got = {"y": d.results(eng)["y"]}
    got.update({k: v for k, v in run(eng, c, y=y32).items() if k != "y"})
    assert sorted(got) == sorted(ref)
    worst = {}
    for k in ref:
        assert got[k].shape == ref[k].shape and np.isfinite(got[k]).all(), (name, k)
        r = S.ratio(got[k], ref[k], bound[k])
        worst[S.KERNEL_OF(k)] = max(worst.get(S.KERNEL_OF(k), 0.0), r)
    for kernel, r in worst.items():
        RATIOS[kernel] = max(RATIOS.get(kernel, 0.0), r)
        print("%-16s %-8s largest |gpu - ref64| / bound = %.3f   (so far: %.3f)" % (name, kernel, r, RATIOS[kernel]))
    for k in ref:
        r = S.ratio(got[k], ref[k], bound[k])
        assert r <= 1.0, (name, k, r)


# ---- 4. the autograd function on reference-shaped modules against eager torch in float32
def _modules(shape, seed):
    """conv_q1 or conv_b1_1..3 as the nets build them (Model_QBD.py:68, :108-110), with torch's default initialisation."""
    torch.manual_seed(seed)
    return [torch.nn.Conv2d(s[1], s[0], kernel_size=(s[2], s[3]), padding=0, stride=1).cuda() for s in S.conv_shapes(shape)]


@pytest.mark.parametrize("shape,x_grad", [((2, 16, 32, 1, 9, 0), False), ((2, 32, 16, 2, 9, 1), True), ((1, 16, 16, 3, 5, 0), True),
                                          ((3, 16, 16, 4, 5, 1), False)])
def test_stem_of_modules_against_eager_torch(eng, shape, x_grad):
    from pmp_vvc_tip2023_amd import stem
    n, h, w, cin, k, split = shape
    p = k // 2
    mods = _modules(shape, 7 + cin)
    g = torch.Generator().manual_seed(100 + cin)
    x0 = torch.randn((n, cin, h + p, w + p), generator=g).cuda()
    g_y = torch.randn((n, 32, h, w), generator=g).cuda()

    def grads(x, ms):
        torch.cuda.synchronize()
        r = {"g_x": None if x.grad is None else x.grad.cpu().numpy()}
        for j, m in enumerate(ms):
            r["g_w%d" % j], r["g_b%d" % j] = m.weight.grad.cpu().numpy(), m.bias.grad.cpu().numpy()
        return r

    try:
        x = x0.clone().requires_grad_(x_grad)
        y = stem.stem_of(eng, mods, x)
        y.backward(g_y)
        got = dict(grads(x, mods), y=y.detach().cpu().numpy())
    finally:
        eng.set_stream(0)
    # eager torch in float32, on the CPU: the same modules, the reference's statements
    cpu = copy.deepcopy(mods)
    for m in cpu:
        m.cpu()
        m.weight.grad = m.bias.grad = None
    x = x0.cpu().clone().requires_grad_(x_grad)
    y = torch.cat([F.relu(m(F.pad(x, pd))) for m, pd in zip(cpu, S.pads(shape))], 1)
    y.backward(g_y.cpu())
    want = dict(grads(x, cpu), y=y.detach().numpy())
    assert (got["g_x"] is not None) == x_grad and (want["g_x"] is not None) == x_grad
    c = {"shape": shape, "x": x0.cpu().numpy(), "g_y": g_y.cpu().numpy(), "w": [m.weight.detach().cpu().numpy() for m in mods],
         "b": [m.bias.detach().cpu().numpy() for m in mods]}
    y64 = S.forward(c)
    ref = S.flat(dict(S.backward(c, got["y"]), y=y64))
    A = S.flat(dict(S.backward(c, got["y"], absolute=True), y=S.forward(c, absolute=True)))
    assert np.array_equal(got["y"] > 0, want["y"] > 0), "the two masks differ: the comparison of the gradients would be void"
    for key in ref:
        if key == "g_x" and not x_grad:
            continue
        bound = S.C_OF[S.KERNEL_OF(key)] * S.EPS * A[key] + S.R_STORE * np.abs(ref[key])
        assert got[key].shape == want[key].shape == ref[key].shape and np.abs(want[key]).max() > 0, key
        r = float(np.where(got[key] == want[key], 0.0, np.abs(got[key].astype(np.float64) - want[key]) / bound).max())
        print("%s %-5s largest |ours - eager| / bound = %.3f" % (shape, key, r))
        assert r <= 1.0, (shape, key, r)


# ---- 5. refusals: PMP_E_INVALID before any launch, nothing written (the matrix of csrc/train_check_main.cpp, through the C ABI)
def test_refusals_write_nothing(eng):
    from pmp_vvc_tip2023_amd import _lib
    cs = {nm: S.exact(nm)[0] for nm in ("q_luma_one", "parts1")}            # one convolution / three
    dev = {nm: Dev(c) for nm, c in cs.items()}
    ok = Dev(cs["q_luma_one"])                                              # a finished forward, for the backward calls
    ok.forward(eng)
    eng.synchronize()
    y_ok = ok.y.clone()
    spare = nan(4096)
    arr = lambda ps: (C.c_void_p * 3)(*ps)

    def call(nm, what, shape=None, null_shape=False, null=(), w=None, b=None, g_w=None, g_b=None, **swap):
        d = ok if what == "backward" and nm == "q_luma_one" else dev[nm]
        p = {"x": P(d.x), "y": P(d.y), "g_y": P(d.g_y), "g_x": P(d.g_x)}
        p.update(swap)
        arrays = {}
        for key, tensors, change in (("w", d.w, w), ("b", d.b, b), ("g_w", d.g_w, g_w), ("g_b", d.g_b, g_b)):
            ptrs = [P(a) for a in tensors] + [None] * (3 - len(tensors))
            for i, v in (change or {}).items():
                ptrs[i] = v
            arrays[key] = None if key in null else arr(ptrs)
        s = _lib.stem_shape(shape or d.shape)
        sp = None if null_shape else C.byref(s)
        if what == "forward":
            return eng.lib.pmp_stem_forward_device(eng.h, sp, p["x"], arrays["w"], arrays["b"], p["y"])
        return eng.lib.pmp_stem_backward_device(eng.h, sp, p["x"], p["y"], arrays["w"], p["g_y"], p["g_x"], arrays["g_w"], arrays["g_b"])

    bad_shapes = [(0, 16, 16, 1, 9, 0), (257, 16, 16, 1, 9, 0), (-1, 16, 16, 1, 9, 0), (1, 8, 16, 1, 9, 0), (1, 24, 16, 1, 9, 0),
                  (1, 272, 16, 1, 9, 0), (1, -16, 16, 1, 9, 0), (1, 16, 0, 1, 9, 0), (1, 16, 40, 1, 9, 0), (1, 16, 272, 1, 9, 0),
                  (1, 16, 16, 0, 9, 0), (1, 16, 16, 5, 9, 0), (1, 16, 16, -1, 9, 0), (1, 16, 16, 1, 3, 0), (1, 16, 16, 1, 7, 0),
                  (1, 16, 16, 1, 4, 0), (1, 16, 16, 1, 11, 0), (1, 16, 16, 1, -9, 0), (1, 16, 16, 1, 9, 2), (1, 16, 16, 1, 9, -1)]
    q, m = dev["q_luma_one"], dev["parts1"]
    tries = []
    for what in ("forward", "backward"):
        tries += [("shape %s" % (s,), "q_luma_one", what, dict(shape=s)) for s in bad_shapes]
        tries += [("null shape", "q_luma_one", what, dict(null_shape=True)), ("null d_w", "q_luma_one", what, dict(null=("w",))),
                  ("null w[0]", "q_luma_one", what, dict(w={0: None})), ("null w[0], split", "parts1", what, dict(w={0: None})),
                  ("w[1] without split", "q_luma_one", what, dict(w={1: P(spare)})),
                  ("w[1] and w[2] without split", "q_luma_one", what, dict(w={1: P(m.w[1]), 2: P(m.w[2])})),
                  ("no w[1] with split", "parts1", what, dict(w={1: None})), ("no w[2] with split", "parts1", what, dict(w={2: None})),
                  ("split = 1 with one tensor", "q_luma_one", what, dict(shape=(1, 16, 16, 1, 9, 1))),
                  ("split = 0 with three tensors", "parts1", what, dict(shape=(1, 16, 16, 4, 9, 0))),
                  ("null x", "q_luma_one", what, dict(x=None)), ("misaligned x", "q_luma_one", what, dict(x=P(q.x) + 2)),
                  ("misaligned w[0]", "q_luma_one", what, dict(w={0: P(q.w[0]) + 1})), ("misaligned w[2]", "parts1", what, dict(w={2: P(m.w[2]) + 2}))]
    tries += [("null d_b", "q_luma_one", "forward", dict(null=("b",))), ("null b[0]", "parts1", "forward", dict(b={0: None})),
              ("b[2] without split", "q_luma_one", "forward", dict(b={2: P(spare)})), ("no b[1] with split", "parts1", "forward", dict(b={1: None})),
              ("null y", "q_luma_one", "forward", dict(y=None)), ("y overlaps x", "q_luma_one", "forward", dict(y=P(q.x) + 64)),
              ("y overlaps the end of x", "q_luma_one", "forward", dict(y=P(q.x) + 4 * (q.x.numel() - 1))),
              ("y is w[0]", "q_luma_one", "forward", dict(y=P(q.w[0]))), ("y overlaps b[1]", "parts1", "forward", dict(y=P(m.b[1]) - 4 * 100)),
              ("misaligned y", "q_luma_one", "forward", dict(y=P(q.y) + 2)), ("misaligned b[0]", "q_luma_one", "forward", dict(b={0: P(q.b[0]) + 2})),
              ("null y", "q_luma_one", "backward", dict(y=None)), ("null g_y", "q_luma_one", "backward", dict(g_y=None)),
              ("null d_g_w", "q_luma_one", "backward", dict(null=("g_w",))), ("null d_g_b", "q_luma_one", "backward", dict(null=("g_b",))),
              ("null g_w[0]", "q_luma_one", "backward", dict(g_w={0: None})), ("null g_b[0]", "parts1", "backward", dict(g_b={0: None})),
              ("g_w[1] without split", "q_luma_one", "backward", dict(g_w={1: P(spare)})),
              ("g_b[2] without split", "q_luma_one", "backward", dict(g_b={2: P(spare)})),
              ("no g_w[2] with split", "parts1", "backward", dict(g_w={2: None})), ("no g_b[1] with split", "parts1", "backward", dict(g_b={1: None})),
              ("g_x overlaps x", "q_luma_one", "backward", dict(g_x=P(ok.x) + 16)), ("g_x is g_y", "q_luma_one", "backward", dict(g_x=P(ok.g_y))),
              ("g_x inside y", "q_luma_one", "backward", dict(g_x=P(ok.y) + 1024)), ("g_w[0] is w[0]", "q_luma_one", "backward", dict(g_w={0: P(ok.w[0])})),
              ("g_w[0] overlaps g_x", "q_luma_one", "backward", dict(g_w={0: P(ok.g_x) + 16})),
              ("g_b[0] inside g_w[0]", "q_luma_one", "backward", dict(g_b={0: P(ok.g_w[0]) + 64})),
              ("g_w[1] is g_w[2]", "parts1", "backward", dict(g_w={1: P(m.g_w[2])})), ("g_b[1] overlaps g_b[2]", "parts1", "backward", dict(g_b={1: P(m.g_b[2]) - 16})),
              ("g_b[0] overlaps g_y", "q_luma_one", "backward", dict(g_b={0: P(ok.g_y) + 4})),
              ("misaligned g_x", "q_luma_one", "backward", dict(g_x=P(ok.g_x) + 2)), ("misaligned g_y", "q_luma_one", "backward", dict(g_y=P(ok.g_y) + 1)),
              ("misaligned y", "q_luma_one", "backward", dict(y=P(ok.y) + 2)), ("misaligned g_w[0]", "q_luma_one", "backward", dict(g_w={0: P(ok.g_w[0]) + 2})),
              ("misaligned g_b[2]", "parts1", "backward", dict(g_b={2: P(m.g_b[2]) + 2}))]
    R.refuse_all(eng, tries, call)
    for nm, d in dev.items():
        R.check_untouched(nm, d.outputs(), d.inputs(cs[nm]))
    R.check_untouched("ok", ok.outputs(), ok.inputs(cs["q_luma_one"]), skip=("y",))                # its forward ran
    assert torch.isnan(spare).all() and torch.equal(ok.y, y_ok)
    # and the calls after a refusal still work
    ok.backward(eng)
    check_bits("after the refusals", ok.results(eng), S.exact("q_luma_one")[1])
