"""GPU: one ResidualBlock, forward and backward (include/pmp.h: pmp_resblock_forward / pmp_resblock_backward; csrc/api_train.cpp,
conv_wgrad.hip; pmp_vvc_tip2023_amd/resblock.py).

Bounds.  On the EXACT cases of tests/resblock_cases.py every value is an integer below 2^24, float32 arithmetic is exact in any order,
and every output must equal the float64 restatement BIT FOR BIT, no element left out - in poisoned workspaces and into buffers
pre-filled with NaN, so an unwritten partial sum or padded channel shows.  On the FLOAT cases the kernel's error against float64,
E = max |result - f64| / max |f64| per tensor, must be at most 4 x the E of torch's own CPU float32 ops on the same inputs: the factor
covers a different but equally valid float32 order of summation.  `pytest -s` prints the measured ratios."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import resblock_cases as K
import train_rig as R

pytestmark = pytest.mark.gpu

FWD_IN, BWD_IN, GRADS = R.FWD_IN, R.BWD_IN, R.GRADS
P, up, nan_dev, shape_of, check_bits = R.P, R.up, R.nan_dev, R.shape_of, R.check_bits
dev_forward, dev_backward, host_calls, _np = R.dev_forward, R.dev_backward, R.host_calls, R._np
eng = R.engine_fixture()


@functools.lru_cache(maxsize=None)
def exact(name):
    """-> (case with t and out as float32, the float64 restatement as the float32 a kernel must produce); computed once, never changed."""
    c = K.make_exact(name)
    want = {k: K.as_f32(v) for k, v in K.restate(c).items()}
    c["t"], c["out"] = want["t"], want["out"]
    return c, want


# ---- 1. every exact case, device and host form, in poisoned workspaces, into NaN-filled buffers
@pytest.mark.parametrize("name", list(K.EXACT))
def test_exact_cases_bit_equal(eng, name):
    c, want = exact(name)
    for pattern in (1, 2):
        eng._ck(eng.lib.pmp_debug_poison_workspace(eng.h, pattern))
        check_bits("device forward, poison %d" % pattern, dev_forward(eng, c), want, ("t", "out"))
        check_bits("device backward, poison %d" % pattern, dev_backward(eng, c), want, GRADS)
        rf, rb, o = host_calls(eng, c)
        assert rf == 0 and rb == 0, (rf, rb, eng.lib.pmp_last_error(eng.h))
        check_bits("host, poison %d" % pattern, o, want, ("t", "out") + GRADS)
    eng._ck(eng.lib.pmp_debug_poison_workspace(eng.h, 0))
    t, out = eng.resblock_forward(c["x"], c["w0"], c["w2"], c["wsc"])                 # the Engine's own host wrappers
    g = dict(zip(GRADS, eng.resblock_backward(c["x"], t, out, c["w0"], c["w2"], c["wsc"], c["g_out"])))
    check_bits("Engine", dict(g, t=t, out=out), want, ("t", "out") + GRADS)


# ---- 2. the forward pass is the inference graph's on PMP_PRECISION_F32: pins the device packer to the loader's packing
class RBCase(C.Structure):
    _fields_ = [(f, C.c_int) for f in ("n", "h", "w", "cin", "cout", "k", "gate", "pool", "out_f32", "exp_x", "exp_gate", "exp_out")]


@pytest.mark.parametrize("name", ["identity", "sc_5x5", "c64_5x5", "c64_32", "prime_n", "f_sc_5x5"])
def test_forward_equals_inference_graph(eng, name):
    from oracle import taps as T
    from pmp_vvc_tip2023_amd import engine
    c = K.make_float(name) if name in K.FLOAT else K.make_exact(name)
    n, h, w, cin, cout, k = c["shape"]
    got = dev_forward(eng, c)
    e2 = engine.Engine(0)
    try:
        e2.set_precision("fp32")
        T.taps_on(e2, True)
        cs = RBCase(n, h, w, cin, cout, k, 0, 0, 0, 0, 0, 0)
        fp = lambda a: None if a is None else np.ascontiguousarray(a, np.float32).ctypes.data_as(C.POINTER(C.c_float))
        keep = [np.ascontiguousarray(c[key], np.float32) if c[key] is not None else None for key in FWD_IN]
        e2._ck(e2.lib.pmp_debug_run_resblock(e2.h, C.byref(cs), *[fp(a) for a in keep], None, None, None, 0))
        for tap, key in (("rb.t", "t"), ("rb", "out")):
            a, c_real = T.tap(e2, tap)
            assert c_real == cout
            assert K.same_bits(a[:, :cout].astype(np.float32), got[key]), (name, tap)
    finally:
        e2.close()


# ---- 3. g_x = NULL: not computed, and the weight gradients are the same
@pytest.mark.parametrize("name", ["identity", "padded_cin"])
def test_without_g_x(eng, name):
    c, want = exact(name)
    g = dev_backward(eng, c, want_g_x=False)
    assert np.isnan(g["g_x"]).all()
    check_bits("no g_x", g, want, GRADS[1:])
    gx, gw0, gw2, gwsc = eng.resblock_backward(c["x"], c["t"], c["out"], c["w0"], c["w2"], c["wsc"], c["g_out"], want_g_x=False)
    assert gx is None
    check_bits("Engine, no g_x", {"g_w0": gw0, "g_w2": gw2, "g_wsc": gwsc}, want, GRADS[1:])


# ---- 4. refusals: PMP_E_INVALID before any launch, nothing written
def test_refusals_write_nothing(eng):
    from pmp_vvc_tip2023_amd import _lib
    base = {"identity": exact("identity")[0], "padded_cout": exact("padded_cout")[0]}
    dev = {nm: dict({k: up(c[k]) for k in BWD_IN}, **nan_dev(c, GRADS)) for nm, c in base.items()}
    for nm, c in base.items():
        dev[nm].update(t_o=R.nan(*shape_of(c, "t")), out_o=R.nan(*shape_of(c, "out")))
    R.torch_done()

    def call(nm, which, shape=None, null_shape=False, **swap):
        """The device form of case nm with some pointers swapped (name -> pointer or None) -> return code."""
        d = dev[nm]
        p = {k: P(d[k]) for k in d}
        if base[nm]["wsc"] is None:
            p["wsc"] = p["g_wsc"] = None
        p.update(swap)
        s = _lib.RbShape(*(shape or base[nm]["shape"]))
        sp = None if null_shape else C.byref(s)
        if which == "forward":
            return eng.lib.pmp_resblock_forward_device(eng.h, sp, p["x"], p["w0"], p["w2"], p["wsc"], p["t_o"], p["out_o"])
        return eng.lib.pmp_resblock_backward_device(eng.h, sp, p["x"], p["t"], p["out"], p["w0"], p["w2"], p["wsc"], p["g_out"], p["g_x"], p["g_w0"],
                                                    p["g_w2"], p["g_wsc"])

    n, h, w, cin, cout, k = base["identity"]["shape"]
    bad_shapes = [(0, h, w, cin, cout, k), (257, h, w, cin, cout, k), (n, 8, w, cin, cout, k), (n, 24, w, cin, cout, k), (n, 272, w, cin, cout, k),
                  (n, h, 0, cin, cout, k), (n, h, 40, cin, cout, k), (n, h, 272, cin, cout, k), (n, h, w, 0, cout, k), (n, h, w, 65, cout, k),
                  (n, h, w, cin, 0, k), (n, h, w, cin, 65, k), (n, h, w, cin, cout, 1), (n, h, w, cin, cout, 4), (n, h, w, cin, cout, 7),
                  (n, h, w, cin, 8, k)]                                   # the last: cin != cout without the shortcut's tensors
    idn, pc = dev["identity"], dev["padded_cout"]
    tries = []
    for which in ("forward", "backward"):
        tries += [("shape %s" % (s,), "identity", which, dict(shape=s)) for s in bad_shapes]
        tries += [("null shape", "identity", which, dict(null_shape=True)), ("null x", "identity", which, dict(x=None)),
                  ("null w0", "identity", which, dict(w0=None)), ("null w2", "identity", which, dict(w2=None)),
                  ("wsc with an identity shortcut", "identity", which, dict(wsc=P(pc["wsc"]))),
                  ("no wsc with a conv shortcut", "padded_cout", which, dict(wsc=None)),
                  ("misaligned x", "identity", which, dict(x=P(idn["x"]) + 2))]
    tries += [("null t out", "identity", "forward", dict(t_o=None)), ("null out out", "identity", "forward", dict(out_o=None)),
              ("t overlaps x", "identity", "forward", dict(t_o=P(idn["x"]) + 64)),
              ("t is out", "identity", "forward", dict(out_o=P(idn["t_o"]))),
              ("out overlaps w2", "identity", "forward", dict(out_o=P(idn["w2"]))),
              ("misaligned out", "identity", "forward", dict(out_o=P(idn["out_o"]) + 1)),
              ("null t", "identity", "backward", dict(t=None)), ("null out", "identity", "backward", dict(out=None)),
              ("null g_out", "identity", "backward", dict(g_out=None)),
              ("null g_w0", "identity", "backward", dict(g_w0=None)), ("null g_w2", "identity", "backward", dict(g_w2=None)),
              ("g_wsc with an identity shortcut", "identity", "backward", dict(g_wsc=P(pc["g_wsc"]))),
              ("no g_wsc with a conv shortcut", "padded_cout", "backward", dict(g_wsc=None)),
              ("g_x overlaps g_out", "identity", "backward", dict(g_x=P(idn["g_out"]))),
              ("g_w0 is g_w2", "identity", "backward", dict(g_w0=P(idn["g_w2"]))),
              ("g_w2 overlaps t", "identity", "backward", dict(g_w2=P(idn["t"]) + 4)),
              ("misaligned g_w0", "identity", "backward", dict(g_w0=P(idn["g_w0"]) + 2))]
    R.refuse_all(eng, tries, call)
    for nm, c in base.items():                                             # ... and the inputs are what they were
        R.check_untouched(nm, [(k, dev[nm][k]) for k in ("t_o", "out_o") + GRADS],
                          [(k, dev[nm][k], c[k]) for k in BWD_IN if c[k] is not None])
    # the host forms refuse the same way
    c = base["identity"]
    s = _lib.RbShape(n, h, w, cin, cout, 4)
    a = {k: None if c[k] is None else np.ascontiguousarray(c[k], np.float32) for k in BWD_IN}
    o = {k: np.full(shape_of(c, k), np.nan, np.float32) for k in ("t", "out") + GRADS[:3]}
    assert eng.lib.pmp_resblock_forward(eng.h, C.byref(s), *[_np(a[k]) for k in FWD_IN], _np(o["t"]), _np(o["out"])) == -1
    s = _lib.RbShape(*c["shape"])
    assert eng.lib.pmp_resblock_forward(eng.h, C.byref(s), *[_np(a[k]) for k in FWD_IN], _np(o["t"]), _np(o["t"])) == -1
    assert eng.lib.pmp_resblock_backward(eng.h, C.byref(s), *[_np(a[k]) for k in BWD_IN], _np(o["g_x"]), _np(o["g_w0"]), None, None) == -1
    assert eng.lib.pmp_resblock_backward(eng.h, C.byref(s), *[_np(a[k]) for k in BWD_IN], _np(a["x"]), _np(o["g_w0"]), _np(o["g_w2"]), None) == -1
    assert all(np.isnan(v).all() for v in o.values())
    # and the calls after a refusal still work
    check_bits("after the refusals", dev_backward(eng, c), exact("identity")[1], GRADS)


# ---- 4b. the workspace a block call needs: what it needed before the block calls shared the trunk's block path, to the byte, at
# a trainer's sizes.  The bounds are pmp_get_workspace_bytes() of these same lines at the commit before that change (a pure host
# function of the shape and the arena's take/give order); a mask or a copy of t kept beside gt would add n * pad(cout) * h * w * 4.
WORKSPACE_NEED = {(64, 64, 64, 32, 64, 3): 235028480, (64, 64, 64, 64, 64, 3): 268582912, (64, 32, 32, 64, 32, 3): 41979904,
                  (48, 32, 32, 32, 64, 5): 64110592}


@pytest.mark.parametrize("shape", list(WORKSPACE_NEED), ids=lambda s: "x".join(map(str, s)))
def test_workspace_need_of_block_calls(shape):
    from pmp_vvc_tip2023_amd import engine
    c = {"shape": shape}
    sc = shape[3] != shape[4]
    d = {k: torch.zeros(shape_of(c, k), device="cuda") if sc or k not in ("wsc", "g_wsc") else None for k in BWD_IN + GRADS}
    e = engine.Engine(0)
    try:
        e.resblock_forward_device(shape, *[P(d[k]) for k in FWD_IN], P(d["t"]), P(d["out"]))
        e.resblock_backward_device(shape, *[P(d[k]) for k in BWD_IN], *[P(d[k]) for k in GRADS])
        e.synchronize()
        need = e.workspace_bytes()
    finally:
        e.close()
    print("workspace need of %s: %d bytes (bound %d)" % (shape, need, WORKSPACE_NEED[shape]))
    assert 0 < need <= WORKSPACE_NEED[shape], (shape, need)


# ---- 5. determinism: twice, on a second stream, on a second context
def test_same_bits_on_every_run_stream_and_context(eng):
    c = K.make_float("f_sc_5x5")
    t64, out64 = K.forward(c["x"], c["w0"], c["w2"], c["wsc"])
    c["t"], c["out"] = K.as_f32(t64), K.as_f32(out64)
    R.same_bits_on_every_run_stream_and_context(eng, R.run_block, c, context_stream=False)


# ---- 6. float values: no further from float64 than 4 x torch's own float32 ops
@pytest.mark.parametrize("name", list(K.FLOAT))
def test_float_case_within_4x_of_torch_float32(eng, name):
    c = K.make_float(name)
    t64, out64 = K.forward(c["x"], c["w0"], c["w2"], c["wsc"])
    c["t"], c["out"] = K.as_f32(t64), K.as_f32(out64)                   # the masks are fixed: float32 roundings of the float64 forward
    ref = dict(K.backward(c["x"], c["t"], c["out"], c["w0"], c["w2"], c["wsc"], c["g_out"]), t=t64, out=out64)
    t32, out32 = K.forward(c["x"], c["w0"], c["w2"], c["wsc"], torch.float32)
    cpu = dict(K.backward(c["x"], c["t"], c["out"], c["w0"], c["w2"], c["wsc"], c["g_out"], torch.float32), t=t32, out=out32)
    got = R.run_block(eng, c)
    worst = []
    for k in K.OUTPUTS:
        if ref[k] is None:
            continue
        assert got[k].shape == ref[k].shape and np.isfinite(got[k]).all(), (name, k)
        mine, theirs = K.rel_err(got[k], ref[k]), K.rel_err(cpu[k], ref[k])
        print("%s %-5s E kernel %.3g, E torch CPU float32 %.3g, ratio %.2f" % (name, k, mine, theirs, mine / theirs))
        worst.append((k, mine, theirs))
    for k, mine, theirs in worst:
        assert mine <= 4 * theirs, (name, k, mine, theirs)


# ---- 7. under torch.autograd, on CUDA tensors
@pytest.mark.parametrize("name", ["padded_cin", "identity"])
def test_autograd_function(eng, name):
    from pmp_vvc_tip2023_amd import resblock
    c, want = exact(name)
    try:
        for x_grad in (True, False):
            m = R.reference_block(c["w0"], c["w2"], c["wsc"]).cuda()
            x = up(c["x"]).requires_grad_(x_grad)
            out = resblock.residual_block_of(eng, m, x)
            out.backward(up(c["g_out"]))
            torch.cuda.synchronize()
            got = {"out": out.detach().cpu().numpy(), "g_x": x.grad.cpu().numpy() if x_grad else None, "g_w0": m.left[0].weight.grad.cpu().numpy(),
                   "g_w2": m.left[2].weight.grad.cpu().numpy(),
                   "g_wsc": m.shortcut[0].weight.grad.cpu().numpy().reshape(shape_of(c, "wsc")) if c["wsc"] is not None else None}
            assert (x.grad is None) == (not x_grad)
            check_bits("autograd, x.requires_grad %s" % x_grad, got, want, ("out",) + (GRADS if x_grad else GRADS[1:]))
        # the bare-tensor form, weights as leaves
        w0, w2, wsc = (None if c[k] is None else up(c[k]).requires_grad_() for k in ("w0", "w2", "wsc"))
        resblock.residual_block(eng, up(c["x"]), w0, w2, wsc).backward(up(c["g_out"]))
        torch.cuda.synchronize()
        check_bits("residual_block", {"g_w0": w0.grad.cpu().numpy(), "g_w2": w2.grad.cpu().numpy(),
                                      "g_wsc": None if wsc is None else wsc.grad.cpu().numpy()}, want, GRADS[1:])
    finally:
        eng.set_stream(0)
