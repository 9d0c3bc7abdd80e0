"""GPU: an MTT net's heads and gate products, forward and backward (include/pmp.h: pmp_head_*, pmp_gate_*; csrc/api_train.cpp,
head_train.hip; pmp_vvc_tip2023_amd/head.py).

Bounds.  On the EXACT cases of tests/head_cases.py every value is an integer and every partial sum is below 2^24: y, att, g_x, g_w, g_b,
g_q and g_prev must equal the float64 restatement BIT FOR BIT, in poisoned workspaces, into NaN-filled outputs, and what is not asked
for stays NaN.  On the FLOAT cases y, g_x, g_w and g_b stay within head_cases' bound
    |gpu - ref64| <= c * 2^-24 * A + 2^-23 * |ref64|,   c = 17.2 (y), 9.2 (g_x), 7.8 (g_w), 5.4 (g_b),
twice what the emulated order of summation reaches; att, g_q and g_prev - copies and chains of float32 additions - equal the emulation
bit for bit, which pins the order of the windows.  The ORDER cases pin the carry behind the bias the same way.  The gate equals numpy's
float32 x * a, g_y * x and g_acc + g_y * a bit for bit.  Largest ratios measured on an MI355X: head_cases' docstring."""
import ctypes as C

import numpy as np
import pytest
import torch

import head_cases as H
import train_rig as R

pytestmark = pytest.mark.gpu
RATIOS = {}
P, nan, up = R.P, R.nan, R.up
eng = R.engine_fixture(poison=1)
HeadDev, IN_F = R.HeadDev, R.HeadDev.IN_F


def run(e, c, off4=False):
    d = HeadDev(c, off4)
    d.forward(e)
    d.backward(e)
    return d.results(e)


def check(what, got, want):
    """Bit for bit where want has a tensor; where the case does not ask (None), the buffer - if there is one - is still NaN."""
    for k, v in want.items():
        if v is None:
            assert k not in got or np.isnan(got[k]).all(), (what, k, "written without being asked for")
        else:
            assert got[k].dtype == np.float32 and H.same_bits(got[k], v), (what, k, np.argwhere(~(got[k] == v))[:4])


# ---- 1. every exact case equals the restatement: poisoned workspaces, NaN-filled outputs, nothing written that was not asked for; the
# second pass with every tensor inside a NaN-guarded allocation of its own, so that a write beyond an output's end shows
@pytest.mark.parametrize("name", list(H.EXACT))
def test_exact_cases_bit_equal(eng, name):
    c, want = H.exact(name)
    try:
        for pattern in (1, 2):
            eng._ck(eng.lib.pmp_debug_poison_workspace(eng.h, pattern))
            d = HeadDev(c, off4=pattern == 2)
            d.forward(eng)
            d.backward(eng)
            check("poison %d" % pattern, d.results(eng), want)
            R.check_untouched(name, [], d.inputs())
    finally:
        eng._ck(eng.lib.pmp_debug_poison_workspace(eng.h, 1))


# g_x, g_q and g_prev are optional one by one, whatever the case has: g_prev without a carry (with and without an attention input),
# everything optional left out, and everything asked for - each output that is not passed stays NaN, the others keep their bits
@pytest.mark.parametrize("name", ["b1_16x24", "one_8x8", "b2_24x16"])
@pytest.mark.parametrize("want_g_x,want_g_q,want_g_prev", [(False, False, True), (True, True, True), (False, False, False)])
def test_optional_outputs_one_by_one(eng, name, want_g_x, want_g_q, want_g_prev):
    c = H.make_case(name)
    want_g_q = want_g_q and c["shape"][6] != 0
    want = {k: H.as_f32(v) for k, v in H.restate(c).items()}
    for k, asked in (("g_x", want_g_x), ("g_q", want_g_q), ("g_prev", want_g_prev)):
        if not asked:
            want[k] = None
    d = HeadDev(c, off4=True)
    d.forward(eng)
    d.backward(eng, want_g_x=want_g_x, want_g_q=want_g_q, want_g_prev=want_g_prev)
    check(name, d.results(eng), want)
    assert not want_g_prev or (np.abs(want["g_prev"][:, 0]).max() > 0 and not want["g_prev"][:, 1:].any())


def test_every_tensor_four_bytes_off_a_16_byte_boundary(eng):
    c, want = H.exact("b2_24x16")
    check("off by 4", run(eng, c, off4=True), want)


def test_same_bits_on_every_run_stream_and_context(eng):
    R.same_bits_on_every_run_stream_and_context(eng, run, H.make_case("f_b2", "randn"), nonzero=True)


# ---- 2. float values: within the bound, and the pure additions equal to the emulation bit for bit
@pytest.mark.parametrize("name", list(H.FLOAT))
def test_float_cases_within_the_bound(eng, name):
    c, ref, bound, A, emu = H.float_reference(name)
    got = run(eng, c)
    for k in H.BOUNDED:
        assert got[k].shape == ref[k].shape and np.isfinite(got[k]).all(), (name, k)
        r = H.ratio(got[k], ref[k], bound[k])
        RATIOS[k] = max(RATIOS.get(k, 0.0), r)
        print("%-14s %-4s largest |gpu - ref64| / bound = %.3f   (so far: %.3f)   equals the emulation: %s" %
              (name, k, r, RATIOS[k], H.same_bits(got[k], emu[k])))
    for k in H.BOUNDED:
        assert H.ratio(got[k], ref[k], bound[k]) <= 1.0, (name, k)
    sz = H.sizes(c["shape"])
    att = np.concatenate([H.up(c["q"], c["shape"][5]), H.up(got["y"], c["shape"][6])], 1)
    assert got["att"].shape == sz["att"] and H.same_bits(got["att"], att), "att is q's and the carried y's bits"
    for k in ("g_q", "g_prev"):
        if k == "g_prev" and c["prev"] is None:
            assert np.isnan(got[k]).all()
        else:
            assert H.same_bits(got[k], emu[k]), (name, k, "the order of the window's additions")


@pytest.mark.parametrize("name", list(H.ORDER))
def test_carry_is_added_behind_the_bias(eng, name):
    c = H.make_case(name, "order")
    d = HeadDev(c)
    d.forward(eng)
    got = d.results(eng)
    want = H.emulate(c)
    assert H.same_bits(got["y"], want["y"]), name
    assert want["att"] is None or H.same_bits(got["att"], want["att"])


# ---- 3. the gate
@pytest.mark.parametrize("count", H.GATE_COUNTS)
@pytest.mark.parametrize("off", [0, 4, 12])
def test_gate_equals_numpy_float32(eng, count, off):
    c = H.gate_case(count, off)
    bufs = {}

    def dev(k, src=None):
        buf = nan(count + 8)
        view = buf[off // 4:off // 4 + count]
        if src is not None:
            view.copy_(up(src))
        bufs[k] = (buf, view)
        assert view.data_ptr() % 16 == off
        return view

    d = {k: dev(k, c[k]) for k in ("x", "a", "g_y", "g_acc")}
    for with_acc in (True, False):
        o = {k: dev(k) for k in ("y", "g_x", "g_a")}
        R.torch_done()
        eng.gate_forward_device(count, P(d["x"]), P(d["a"]), P(o["y"]))
        eng.gate_backward_device(count, P(d["x"]), P(d["a"]), P(d["g_y"]), P(d["g_acc"]) if with_acc else None, P(o["g_x"]), P(o["g_a"]))
        eng.synchronize()
        want = H.gate_reference(c, with_acc)
        for k, v in want.items():
            assert H.same_bits(R.num(o[k]), v), (count, off, with_acc, k)
            buf = bufs[k][0]
            assert torch.isnan(buf[:off // 4]).all() and torch.isnan(buf[off // 4 + count:]).all(), (k, "written outside the output")
    for k in d:
        assert H.same_bits(R.num(d[k]), c[k]), (k, "an input changed")


# ---- 4. refusals: PMP_E_INVALID before any launch, nothing written
def test_refusals_write_nothing(eng):
    from pmp_vvc_tip2023_amd import _lib
    cs = {nm: H.exact(nm)[0] for nm in ("b3_16x16", "b2_24x16")}                # without / with an attention input
    dev = {nm: HeadDev(c) for nm, c in cs.items()}
    spare = nan(65536)

    def call(nm, what, shape=None, null_shape=False, **swap):
        d = dev[nm]
        p = {k: P(t) for k, t in list(d.d.items()) + list(d.o.items())}
        for k in ("att", "g_q"):
            p.setdefault(k, None)
        p.update(swap)
        s = _lib.head_shape(shape or d.shape)
        sp = None if null_shape else C.byref(s)
        if what == "forward":
            return eng.lib.pmp_head_forward_device(eng.h, sp, p["x"], p["w"], p["b"], p["prev"], p["q"], p["y"], p["att"])
        return eng.lib.pmp_head_backward_device(eng.h, sp, p["x"], p["w"], p["g_y"], p["g_att"], p["g_x"], p["g_w"], p["g_b"], p["g_q"], p["g_prev"])

    plain, att = dev["b3_16x16"], dev["b2_24x16"]
    bad_shapes = [(0, 16, 16, 8, 2, 0, 0), (257, 16, 16, 8, 2, 0, 0), (-1, 16, 16, 8, 2, 0, 0), (3, 0, 16, 8, 2, 0, 0), (3, 4, 16, 8, 2, 0, 0),
                  (3, 12, 16, 8, 2, 0, 0), (3, 264, 16, 8, 2, 0, 0), (3, -8, 16, 8, 2, 0, 0), (3, 16, 0, 8, 2, 0, 0), (3, 16, 20, 8, 2, 0, 0),
                  (3, 16, 264, 8, 2, 0, 0), (3, 16, 16, 0, 2, 0, 0), (3, 16, 16, 17, 2, 0, 0), (3, 16, 16, -1, 2, 0, 0), (3, 16, 16, 8, 0, 0, 0),
                  (3, 16, 16, 8, 3, 0, 0), (3, 16, 16, 8, -1, 0, 0), (3, 16, 16, 8, 2, 2, 2), (3, 16, 16, 8, 2, 4, 1), (3, 16, 16, 8, 2, 0, 1),
                  (3, 16, 16, 8, 2, 2, 0), (3, 16, 16, 8, 2, 1, 1), (3, 16, 16, 8, 2, 8, 4), (3, 16, 16, 8, 2, -2, -1)]
    tries = []
    for what in ("forward", "backward"):
        tries += [("shape %s" % (s,), "b3_16x16", what, dict(shape=s)) for s in bad_shapes]
        tries += [("null shape", "b3_16x16", what, dict(null_shape=True)), ("null x", "b3_16x16", what, dict(x=None)),
                  ("null w", "b2_24x16", what, dict(w=None)), ("misaligned x", "b3_16x16", what, dict(x=P(plain.d["x"]) + 2)),
                  ("misaligned w", "b2_24x16", what, dict(w=P(att.d["w"]) + 1))]
    tries += [("null b", "b3_16x16", "forward", dict(b=None)), ("null y", "b3_16x16", "forward", dict(y=None)),
              ("q without up_y", "b3_16x16", "forward", dict(q=P(spare))), ("att without up_y", "b3_16x16", "forward", dict(att=P(spare))),
              ("q and att without up_y", "b3_16x16", "forward", dict(q=P(att.d["q"]), att=P(spare))),
              ("up_y without q", "b2_24x16", "forward", dict(q=None)), ("up_y without att", "b2_24x16", "forward", dict(att=None)),
              ("y overlaps x", "b3_16x16", "forward", dict(y=P(plain.d["x"]) + 64)), ("y is prev", "b3_16x16", "forward", dict(y=P(plain.d["prev"]))),
              ("y overlaps the end of w", "b3_16x16", "forward", dict(y=P(plain.d["w"]) + 4 * 143)),
              ("att overlaps q", "b2_24x16", "forward", dict(att=P(att.d["q"]) - 16)), ("att is y", "b2_24x16", "forward", dict(att=P(att.o["y"]))),
              ("misaligned y", "b3_16x16", "forward", dict(y=P(plain.o["y"]) + 2)), ("misaligned prev", "b3_16x16", "forward", dict(prev=P(plain.d["prev"]) + 2)),
              ("misaligned att", "b2_24x16", "forward", dict(att=P(att.o["att"]) + 1)),
              ("null g_y", "b3_16x16", "backward", dict(g_y=None)), ("null g_w", "b3_16x16", "backward", dict(g_w=None)),
              ("null g_b", "b2_24x16", "backward", dict(g_b=None)), ("g_att without up_y", "b3_16x16", "backward", dict(g_att=P(spare))),
              ("up_y without g_att", "b2_24x16", "backward", dict(g_att=None)), ("g_q without g_att", "b3_16x16", "backward", dict(g_q=P(spare))),
              ("g_q and g_att without up_y", "b3_16x16", "backward", dict(g_q=P(att.o["g_q"]), g_att=P(spare))),
              ("g_x is g_y", "b3_16x16", "backward", dict(g_x=P(plain.d["g_y"]))), ("g_x overlaps x", "b3_16x16", "backward", dict(g_x=P(plain.d["x"]) + 16)),
              ("g_w is w", "b3_16x16", "backward", dict(g_w=P(plain.d["w"]))), ("g_b inside g_w", "b3_16x16", "backward", dict(g_b=P(plain.o["g_w"]) + 64)),
              ("g_q inside g_att", "b2_24x16", "backward", dict(g_q=P(att.d["g_att"]) + 1024)), ("g_prev is g_x", "b2_24x16", "backward", dict(g_prev=P(att.o["g_x"]))),
              ("g_prev overlaps g_y", "b3_16x16", "backward", dict(g_prev=P(plain.d["g_y"]) + 4)),
              ("misaligned g_x", "b3_16x16", "backward", dict(g_x=P(plain.o["g_x"]) + 2)), ("misaligned g_att", "b2_24x16", "backward", dict(g_att=P(att.d["g_att"]) + 2)),
              ("misaligned g_q", "b2_24x16", "backward", dict(g_q=P(att.o["g_q"]) + 1)), ("misaligned g_b", "b3_16x16", "backward", dict(g_b=P(plain.o["g_b"]) + 2))]
    R.refuse_all(eng, tries, call)
    # the gate
    a, b, o = spare[:1024], spare[1024:2048], spare[4096:5120]
    gate = [(0, P(a), P(b), P(o)), (-1, P(a), P(b), P(o)), (2 ** 31, P(a), P(b), P(o)), (1024, None, P(b), P(o)), (1024, P(a), None, P(o)),
            (1024, P(a), P(b), None), (1024, P(a), P(b), P(a)), (1024, P(a), P(b), P(b) + 4 * 1023), (1024, P(a) + 2, P(b), P(o)), (1024, P(a), P(b), P(o) + 1)]
    for count, x, g, y in gate:
        assert eng.lib.pmp_gate_forward_device(eng.h, count, x, g, y) == -1 and eng.lib.pmp_last_error(eng.h), (count, x, g, y)
    o2, acc = spare[8192:9216], spare[12288:13312]
    gate_b = [dict(count=0), dict(g_y=None), dict(g_x=None), dict(g_a=None), dict(g_x=P(acc)), dict(g_a=P(o)), dict(g_a=P(a)), dict(g_acc=P(acc) + 2),
              dict(g_x=P(o) + 4 * 512, g_a=P(o))]
    for kw in gate_b:
        p = dict(count=1024, x=P(a), a=P(b), g_y=P(spare[2048:3072]), g_acc=P(acc), g_x=P(o), g_a=P(o2))
        p.update(kw)
        assert eng.lib.pmp_gate_backward_device(eng.h, p["count"], p["x"], p["a"], p["g_y"], p["g_acc"], p["g_x"], p["g_a"]) == -1, kw
        assert eng.lib.pmp_last_error(eng.h), kw
    eng.synchronize()
    torch.cuda.synchronize()
    for nm, d in dev.items():
        R.check_untouched(nm, d.outputs(), d.inputs())
    assert torch.isnan(spare).all()
    # and the calls after a refusal still work
    plain.forward(eng)
    plain.backward(eng)
    check("after the refusals", plain.results(eng), H.exact("b3_16x16")[1])


# ---- 5. head.py under autograd against the float64 restatement
@pytest.mark.parametrize("name,side_stream", [("b1_16x24", False), ("b2_24x16", True), ("b3_16x16", False), ("c16_att1", False)])
def test_head_function_under_autograd(eng, name, side_stream):
    from pmp_vvc_tip2023_amd import head
    c = H.make_case(name)
    want = {k: H.as_f32(v) for k, v in H.restate(c).items()}
    stream = torch.cuda.Stream() if side_stream else torch.cuda.current_stream()
    try:
        with torch.cuda.stream(stream):                                      # a side stream: no host synchronisation in between
            t = {k: None if c[k] is None else up(c[k]).requires_grad_(k in ("x", "w", "b", "prev", "q")) for k in IN_F + ("g_y", "g_att")}
            out = head.head(eng, t["x"], t["w"], t["b"], t["prev"], t["q"], c["shape"][5:])
            y, att = out if c["shape"][6] else (out, None)
            loss = (y * t["g_y"]).sum() if att is None else (y * t["g_y"]).sum() + (att * t["g_att"]).sum()
            loss.backward()
            got = {"y": y.detach(), "att": None if att is None else att.detach(), "g_x": t["x"].grad, "g_w": t["w"].grad, "g_b": t["b"].grad,
                   "g_q": None if t["q"] is None else t["q"].grad, "g_prev": None if t["prev"] is None else t["prev"].grad}
        stream.synchronize()
    finally:
        eng.set_stream(0)
    if c["prev"] is None:
        want["g_prev"] = None
    for k, v in want.items():
        assert (v is None) == (got[k] is None), (name, k)
        assert v is None or H.same_bits(R.num(got[k]), v), (name, k)


def test_head_function_skips_the_gradients_nobody_needs(eng):
    from pmp_vvc_tip2023_amd import head
    c = H.make_case("b2_24x16")
    want = H.exact("b2_24x16")[1]
    try:
        t = {k: up(c[k]) for k in IN_F + ("g_y", "g_att")}
        w, b = t["w"].requires_grad_(), t["b"].requires_grad_()
        y, att = head.head(eng, t["x"], w, b, t["prev"], t["q"], (4, 2))
        ((y * t["g_y"]).sum() + (att * t["g_att"]).sum()).backward()
        torch.cuda.synchronize()
    finally:
        eng.set_stream(0)
    assert H.same_bits(R.num(w.grad), want["g_w"]) and H.same_bits(R.num(b.grad), want["g_b"])
    assert all(t[k].grad is None for k in ("x", "prev", "q"))


def test_gate_function_under_autograd(eng):
    from pmp_vvc_tip2023_amd import head
    c = H.gate_case(1023)
    try:
        x, a = up(c["x"]).view(3, 11, 31).requires_grad_(), up(c["a"]).view(3, 11, 31).requires_grad_()
        y = head.gate(eng, x, a)
        y.backward(up(c["g_y"]).view(3, 11, 31))
        torch.cuda.synchronize()
    finally:
        eng.set_stream(0)
    want = H.gate_reference(c, False)
    assert H.same_bits(R.num(y.detach()).ravel(), want["y"]) and H.same_bits(R.num(x.grad).ravel(), want["g_x"])
    assert H.same_bits(R.num(a.grad).ravel(), want["g_a"])
