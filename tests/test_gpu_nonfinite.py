"""GPU: NaN and inf through the training calls (include/pmp.h: NON-FINITE VALUES IN THE TRAINING CALLS), on the cases of
tests/nonfinite_cases.py.  For every tensor a call writes, with R where torch's autograd reference is not finite, L where the library's
result is not finite and S the reach of the planted elements:
  1. detect    R inside L: what torch reports as non-finite, the library reports as non-finite (NaN or inf, either sign)
  2. contain   L inside S: nothing outside the plants' receptive field is disturbed
  3. elsewhere unchanged.  A block: outside S every element is within tests/grad_cases.py's per-element bound of the float64 reference of
     the CLEAN case (the backward pass is given the reference's t and out, as in the other float tests, so the masks are the same), and
     has the bits of the device calls on the clean case.
     Trunk, QT tail and stem: outside S every element has the bits of the library's own run on the clean case - the kernels are
     deterministic and an element outside S reads nothing that depends on a plant, so nothing looser is needed; the clean runs
     themselves are held to the case modules' bounds once per shape (test_clean_runs_within_the_case_modules_bounds).
     Heads: the bits of the call on the clean case, which is head_cases' own float case or bounded here; gate: numpy's float32 bits.
The engine's workspaces are NaN-filled (poison pattern 1) throughout: a kernel that read a word it had not written would now carry that
NaN to an output outside S.  Outputs are NaN-pre-filled too, so rule 1 would pass on an unwritten element; rules 2 and 3 would not."""
import functools

import numpy as np
import pytest
import torch

import conftest  # noqa: F401 - puts tools/ on sys.path
import grad_cases as G
import nonfinite_cases as NF
import resblock_cases as K
import train_rig as R
import trained_like
from oracle import nets_torch as O

pytestmark = pytest.mark.gpu

eng = R.engine_fixture(poison=1)
BLOCK_KEYS = {"t": "t0", "out": "out0", "g_x": "g_x", "g_w0": "g_w0_0", "g_w2": "g_w2_0", "g_wsc": "g_wsc_0"}


def as_block(c):
    n, h, w, cin, blocks, _ = c["shape"]
    w0, w2, wsc = c["blocks"][0]
    return {"shape": (n, h, w, cin) + tuple(blocks[0]), "x": c["x"], "w0": w0, "w2": w2, "wsc": wsc, "g_out": c["g_y"]}


@functools.lru_cache(maxsize=None)
def block_clean(family, shape, overflow):
    """-> (t32, out32, ref, bound) of grad_cases.float_reference on the clean case; computed once, never changed."""
    t32, out32, ref, bound, _ = G.float_reference(as_block(NF._clean(family, shape, overflow)))
    return t32, out32, ref, bound


_block_runs = {}


def block_clean_run(e, family, shape, overflow):
    """the device calls on the clean case, the backward pass from the clean reference's t and out"""
    key = (family, shape, overflow)
    if key not in _block_runs:
        b = as_block(NF._clean(family, shape, overflow))
        b["t"], b["out"] = block_clean(family, shape, overflow)[:2]
        d = R.BlockDev(b)
        d.forward(e)
        d.backward(e)
        _block_runs[key] = d.results(e)
    return _block_runs[key]


def check_rules(name, key, got, R_, S_, clean=None, ref=None, bound=None):
    """rules 1-3 for one tensor; rule 3 against the clean run's bits (clean) or the clean reference and its bound (ref, bound)"""
    L = ~np.isfinite(got)
    assert got.shape == R_.shape == S_.shape, (name, key)
    print("%s %-8s |R| %6d  |L| %6d  |S| %6d of %d" % (name, key, R_.sum(), L.sum(), S_.sum(), S_.size))
    assert not (R_ & ~L).any(), (name, key, "torch reports a non-finite value, the library a finite one", np.argwhere(R_ & ~L)[:4].tolist())
    assert not (L & ~S_).any(), (name, key, "non-finite outside the plant's reach", np.argwhere(L & ~S_)[:4].tolist())
    out = ~S_
    if clean is not None:
        assert K.same_bits(got[out], clean[out]), (name, key, "changed outside the plant's reach", np.argwhere(out & (got != clean))[:4].tolist())
    else:
        err = np.abs(got.astype(np.float64) - ref)
        assert (err[out] <= bound[out]).all(), (name, key, "outside the plant's reach", float((err[out] / bound[out]).max()))


# ---- one ResidualBlock: device and host form
@pytest.mark.parametrize("name", [nm for nm, v in NF.CASES.items() if v[0] == "block"])
def test_block(eng, name):
    family, shape, plant = NF.CASES[name]
    c = NF.make(name)
    ref = NF.reference(c, NF.reference_dtype(name))
    R_, S_ = NF.footprints(ref), NF.reach(name)
    t32, out32, cref, cbound = block_clean(family, shape, plant == "overflow")
    b = as_block(c)
    # the backward pass is given the reference's t and out: the planted case's inside the reach, the clean case's (the same) outside
    b["t"], b["out"] = np.where(S_["t0"], K.as_f32(ref["t0"]), t32), np.where(S_["out0"], K.as_f32(ref["out0"]), out32)
    d = R.BlockDev(b)
    d.forward(eng)
    d.backward(eng)
    got = d.results(eng)
    base = block_clean_run(eng, family, shape, plant == "overflow")
    rf, rb, host = R.host_calls(eng, b)
    assert rf == 0 and rb == 0, (rf, rb, eng.lib.pmp_last_error(eng.h))
    for form, res in (("device", got), ("host", host)):
        for key, flat in BLOCK_KEYS.items():
            if key == "g_wsc" and b["wsc"] is None:
                continue
            check_rules("%s %s" % (name, form), key, res[key], R_[flat], S_[flat], ref=cref[key], bound=cbound[key])
            assert K.same_bits(res[key][~S_[flat]], base[key][~S_[flat]]), (name, form, key, "not the clean run's bits outside the plant's reach")


def own_outputs_run(e, b):
    """forward, then backward on the t and out that forward call wrote -> results"""
    d = R.BlockDev(dict(b, t=np.zeros(R.shape_of(b, "t"), np.float32), out=np.zeros(R.shape_of(b, "out"), np.float32)))
    d.forward(e)
    e.synchronize()
    d.d["t"].copy_(d.o["t"])
    d.d["out"].copy_(d.o["out"])
    R.torch_done()
    d.backward(e)
    return d.results(e)


@pytest.mark.parametrize("plant", ["nan_seam", "pinf", "ninf", "pair", "overflow"])
def test_block_backward_on_the_forward_calls_own_outputs(eng, plant):
    """What a trainer does: the library's own footprint of t and out - larger than torch's where an inf became NaN in a padded lane -
    goes into the backward call.  Rules 1 and 2 against autograd, rule 3 against the same two calls on the clean case."""
    family, shape = "block", NF.SHAPES["block"][0]                 # 3 -> 17: padded cin and cout, the 1x1 shortcut
    name = NF.case_id(family, shape, plant)
    R_, S_ = NF.footprints(NF.reference(NF.make(name), NF.reference_dtype(name))), NF.reach(name)
    got, base = own_outputs_run(eng, as_block(NF.make(name))), own_outputs_run(eng, as_block(NF.clean(name)))
    assert all(np.isfinite(v).all() for v in base.values())
    for key, flat in BLOCK_KEYS.items():
        check_rules(name + " own t, out", key, got[key], R_[flat], S_[flat], clean=base[key])


# ---- trunk (its saved tensors through pmp_trunk_unpack_device), QT tail, stem: the device forms
RUN = {"trunk": R.run_trunk, "qtail": R.TailDev.run, "stem": lambda e, c: R.run_stem(e, c)}
_clean_runs = {}


def clean_run(e, name):
    family, shape, plant = NF.CASES[name]
    key = (family, shape, plant == "overflow")
    if key not in _clean_runs:
        got = RUN[family](e, NF.clean(name))
        assert all(np.isfinite(v).all() for v in got.values()), (name, "the clean case is not finite")
        _clean_runs[key] = got
    return _clean_runs[key]


@pytest.mark.parametrize("name", [nm for nm, v in NF.CASES.items() if v[0] != "block"])
def test_chain_and_stem(eng, name):
    family = NF.CASES[name][0]
    c = NF.make(name)
    R_, S_ = NF.footprints(NF.reference(c, NF.reference_dtype(name))), NF.reach(name)
    base = clean_run(eng, name)
    got = RUN[family](eng, c)
    if family == "trunk":
        assert K.same_bits(got.pop("x"), c["x"]), (name, "unpack of x")
    assert sorted(got) == sorted(R_), name
    for key in sorted(got):
        check_rules(name, key, got[key], R_[key], S_[key], clean=base[key])


# ---- the heads (attention input, carry, up-sampling; forward and backward) and the gate
def run_head(e, c):
    d = R.HeadDev(c)
    d.forward(e)
    d.backward(e)
    return d.results(e)


_head_clean = {}


@pytest.mark.parametrize("name", list(NF.HEAD_CASES))
def test_head(eng, name):
    """Rules 1 and 2 against autograd; rule 3: outside S the bits of the call on the clean case, which for f_b1 and f_b2 is head_cases'
    f_b1_randn / f_b2_randn - the cases tests/test_gpu_head_grad.py bounds - and for the 8x8 map is bounded here the same way."""
    import head_cases as H
    nm = NF.HEAD_CASES[name][0]
    c = NF.head_make(name)
    ref, S_ = H.asked(c, NF.head_reference(c)), NF.head_reach(name)
    if nm not in _head_clean:
        clean = NF.head_clean(name)
        base = run_head(eng, clean)
        r64, A = H.restate(clean), H.restate(clean, absolute=True)
        for k in H.BOUNDED:
            assert H.ratio(base[k], r64[k], H.C_OF[k] * H.EPS * A[k] + H.R_STORE * np.abs(r64[k])) <= 1, (nm, k, "the clean run")
        _head_clean[nm] = base
    got = run_head(eng, c)
    for k in H.OUT_KEYS:
        if ref[k] is not None:
            check_rules(name, k, got[k], ~np.isfinite(ref[k]), S_[k], clean=_head_clean[nm][k])


@pytest.mark.parametrize("key,value", NF.GATE_PLANTS, ids=lambda v: str(v))
@pytest.mark.parametrize("count", list(NF.GATE_COUNTS))
def test_gate(eng, count, key, value):
    """Elementwise: the planted element is non-finite in the outputs that read the planted tensor wherever numpy's float32 product is
    (torch's is numpy's), every other element has numpy's bits - head_cases.gate_reference, the yardstick of the gate's own test."""
    import head_cases as H
    c, reads = NF.gate_make(count, key, value)
    at = NF.GATE_COUNTS[count]
    d = {k: R.up(c[k]) for k in ("x", "a", "g_y", "g_acc")}
    for with_acc in (True, False):
        o = {k: R.nan(count) for k in ("y", "g_x", "g_a")}
        R.torch_done()
        eng.gate_forward_device(count, R.P(d["x"]), R.P(d["a"]), R.P(o["y"]))
        eng.gate_backward_device(count, R.P(d["x"]), R.P(d["a"]), R.P(d["g_y"]), R.P(d["g_acc"]) if with_acc else None, R.P(o["g_x"]), R.P(o["g_a"]))
        eng.synchronize()
        with np.errstate(invalid="ignore"):
            want = H.gate_reference(c, with_acc)
        for k, v in want.items():
            got = R.num(o[k])
            S_ = np.zeros(count, bool)
            S_[at] = k in reads and (with_acc or key != "g_acc")
            check_rules("gate %d %s %s" % (count, key, value), k, got, ~np.isfinite(v), S_, clean=v)


# ---- the clean runs that rule 3 compares with are themselves right: these shapes are not all in the other tests' tables
def forward_bound(name, key_t, key_o, x32, blk, got):
    """t and out of one block against grad_cases.float_reference on the input the GPU itself had"""
    w0, w2, wsc = blk
    c = {"shape": None, "x": x32, "w0": w0, "w2": w2, "wsc": wsc, "g_out": np.zeros((x32.shape[0], w0.shape[0]) + x32.shape[2:], np.float32)}
    _, _, ref, bound, _ = G.float_reference(c)
    for key, k in ((key_t, "t"), (key_o, "out")):
        r = G.ratio(got[key], ref[k], bound[k])
        print("%s %-5s |gpu - ref64| / bound %.3f" % (name, key, r))
        assert r <= 1, (name, key, r)


@pytest.mark.parametrize("family,shape", [(f, s) for f in ("trunk", "qtail", "stem") for s in NF.SHAPES[f]], ids=lambda v: NF.case_id("", v, "")[1:-1] if isinstance(v, tuple) else v)
def test_clean_runs_within_the_case_modules_bounds(eng, family, shape):
    """stem: stem_cases' per-element bound, the backward pass from the reference's y (stem_cases.float_reference's lines, for a case that
    is not in its table).  trunk: trunk_cases' yardstick for float values - the chain of block calls, bit for bit - and every block's t and
    out within grad_cases' bound of float64 on the input the GPU had.  QT tail: the same forward bound for its four blocks, the pools
    between them exact; its backward at these shapes is test_gpu_qtail_grad.py's ((2, 16, 16) is in qtail_cases.FLOAT)."""
    import qtail_cases as Q
    import stem_cases as S
    import trunk_cases as T
    name = NF.case_id(family, shape, "nan_corner")
    c = NF.clean(name)
    got = clean_run(eng, name)
    if family == "stem":
        y = S.forward(c)
        y32 = S.as_f32(y)
        ref = S.flat(dict(S.backward(c, y32), y=y))
        A = S.flat(dict(S.backward(c, y32, absolute=True), y=S.forward(c, absolute=True)))
        back = R.run_stem(eng, c, y=y32)
        for key in ref:
            bound = S.C_OF[S.KERNEL_OF(key)] * S.EPS * A[key] + S.R_STORE * np.abs(ref[key])
            r = S.ratio((got if key == "y" else back)[key], ref[key], bound)
            print("%s %-5s |gpu - ref64| / bound %.3f" % (name, key, r))
            assert r <= 1, (name, key, r)
    elif family == "trunk":
        d = R.TrunkDev(eng, c)
        d.forward(eng)
        d.backward(eng)
        ts, outs = d.unpack(eng)
        eng.synchronize()
        mine = d.results(eng, ts, outs)
        want = R.chain(eng, c, ts, outs)
        R.check_bits(name, mine, want)
        x = c["x"]
        for i, blk in enumerate(c["blocks"]):
            forward_bound(name, "t%d" % i, "out%d" % i, x, blk, mine)
            x = mine["out%d" % i]
        assert K.same_bits(mine["y"], T.pool(x) if shape[5] else x)
    else:
        b = c["blocks"]
        forward_bound(name, "s1", "s2", got["s0"], b[0], got)
        forward_bound(name, "s3", "s4", Q.multipool(got["s2"]), b[1], got)
        forward_bound(name, "s5", "s6", got["s4"], b[2], got)
        forward_bound(name, "s7", "s8", T.pool(got["s6"]), b[3], got)
        assert K.same_bits(got["x9"], got["s8"])


# ---- whole nets: a NaN in a parameter or an inf in a pixel reaches the outputs, the loss and the gradients as it does in torch.
# Yardstick: oracle.nets_torch on float64 CPU tensors (test_gpu_msbd_net.py's and test_gpu_q_net.py's weights and inputs); wherever
# its outputs or parameter gradients are not finite, the module's are not.
QP = {"Chroma": 27, "Luma": 22}
N_MSBD, N_Q = 72, 20


@functools.lru_cache(maxsize=None)
def net_weights(kind, comp):
    if kind == "msbd":
        return trained_like.msbd_weights(comp, QP[comp])
    from pmp_vvc_tip2023_amd import weights as W
    return {k: np.asarray(v, np.float32) for k, v in W.load_net_weights(comp + "_Q", QP[comp])[0].items()}


def net_inputs(comp):
    """-> (x, q) float64: fixed-seed pixels / 255 and a QT map in 0..3 (test_gpu_msbd_net.py's)"""
    g = torch.Generator().manual_seed(9100 + QP[comp])
    x = torch.randint(0, 256, (1, 1, 68, 68) if comp == "Luma" else (1, 3, 34, 34), generator=g).double() / 255
    return x, torch.randint(0, 4, (1, 1, 8, 8), generator=g).double()


def labels():
    g = torch.Generator().manual_seed(77)
    qt8 = torch.randint(0, 4, (1, 8, 8), generator=g).to(torch.uint8).cuda()
    msbt = torch.randint(0, 4, (1, 3, 16, 16), generator=g).to(torch.uint8).cuda()
    return qt8, msbt, (torch.randint(0, 3, (1, 3, 16, 16), generator=g) - 1).to(torch.int8).cuda()


def planted(wts, key):
    """the weight dict with a NaN in element 0 of wts[key] (key None: unchanged)"""
    w = {k: v.copy() for k, v in wts.items()}
    if key is not None:
        w[key].reshape(-1)[0] = np.nan
    return w


def build(eng, kind, comp, w):
    from pmp_vvc_tip2023_amd import msbd_net, q_net
    net = (msbd_net.MSBDNet if kind == "msbd" else q_net.QNet)(eng, comp == "Luma").cuda()
    net.load_state_dict({k: torch.from_numpy(v) for k, v in w.items()})
    return net


def oracle_forward(kind, comp, w, x, q, grad=False):
    wt = {k: torch.from_numpy(v).double().requires_grad_(grad) for k, v in w.items()}
    luma = comp == "Luma"
    outs = list(O.msbd_forward(wt, x, q, luma)) if kind == "msbd" else [O.q_forward(wt, x, luma)]
    return wt, outs


def outputs_detect(what, outs, ref):
    hit = False
    for i, (o, r) in enumerate(zip(outs, ref)):
        L, R_ = ~torch.isfinite(o.detach().cpu()).numpy(), ~torch.isfinite(r.detach()).numpy()
        assert L.shape == R_.shape and not (R_ & ~L).any(), (what, "output %d" % i, int((R_ & ~L).sum()), "elements are non-finite in torch only")
        hit = hit or R_.any()
    return hit


@pytest.mark.parametrize("index", range(N_MSBD))
def test_nan_in_each_mtt_parameter_reaches_outputs_and_loss(eng, index):
    from pmp_vvc_tip2023_amd import train_loss
    comp = "Chroma"
    wts = net_weights("msbd", comp)
    assert len(wts) == N_MSBD
    key = sorted(wts)[index]
    w = planted(wts, key)
    x, q = net_inputs(comp)
    with torch.no_grad():
        _, ref = oracle_forward("msbd", comp, w, x, q)
    _, msbt, msdire = labels()
    try:
        with torch.no_grad():
            outs = build(eng, "msbd", comp, w)(x.float().cuda(), q.float().cuda())
            loss = train_loss.loss_func_MSBD(eng, *outs, msbt, msdire, False, QP[comp])
        torch.cuda.synchronize()
    finally:
        eng.set_stream(0)
    hit = outputs_detect(key, outs, ref)
    assert hit, (key, "the oracle's outputs are finite: the plant tests nothing")
    assert not np.isfinite(float(loss)), (key, float(loss))


@pytest.mark.parametrize("index", range(N_Q))
def test_nan_in_each_qt_parameter_reaches_output_and_loss(eng, index):
    from pmp_vvc_tip2023_amd import train_loss
    comp = "Chroma"
    wts = net_weights("q", comp)
    assert len(wts) == N_Q
    key = sorted(wts)[index]
    w = planted(wts, key)
    x, _ = net_inputs(comp)
    with torch.no_grad():
        _, ref = oracle_forward("q", comp, w, x, None)
    qt8, _, _ = labels()
    try:
        with torch.no_grad():
            out = build(eng, "q", comp, w)(x.float().cuda())
            loss = train_loss.l1_loss_Q(eng, out, qt8)
        torch.cuda.synchronize()
    finally:
        eng.set_stream(0)
    assert outputs_detect(key, [out], ref), (key, "the oracle's output is finite: the plant tests nothing")
    assert not np.isfinite(float(loss)), (key, float(loss))


@pytest.mark.parametrize("key", ["conv_b1_1.weight", "trunk_M1.2.left.0.weight", "conv_B2.bias"])
def test_backward_detects_what_autograd_does(eng, key):
    comp = "Chroma"
    w = planted(net_weights("msbd", comp), key)
    x, q = net_inputs(comp)
    g = torch.Generator().manual_seed(5)
    gs = [torch.randn((1, 2, 16, 16), generator=g, dtype=torch.float64) for _ in range(3)]
    wt, ref = oracle_forward("msbd", comp, w, x, q, grad=True)
    sum((o * gg).sum() for o, gg in zip(ref, gs)).backward()
    net = build(eng, "msbd", comp, w)
    try:
        outs = net(x.float().cuda(), q.float().cuda())
        sum((o * gg.float().cuda()).sum() for o, gg in zip(outs, gs)).backward()
        torch.cuda.synchronize()
    finally:
        eng.set_stream(0)
    outputs_detect(key, outs, ref)
    params = dict(net.named_parameters())
    some = 0
    for k, v in wt.items():
        R_, L = ~torch.isfinite(v.grad).numpy(), ~torch.isfinite(params[k].grad.cpu()).numpy()
        some += int(R_.any())
        assert not (R_ & ~L).any(), (key, k, int((R_ & ~L).sum()), "gradient elements are non-finite under autograd only")
    assert some, (key, "autograd's gradients are all finite: the plant tests nothing")


def test_inf_pixel_through_the_luma_net(eng):
    """+inf in one pixel of x: the 9x9 stem, trunk_M1's 5x5 block and the pool behind it."""
    comp = "Luma"
    w = planted(net_weights("msbd", comp), None)
    x, q = net_inputs(comp)
    x[0, 0, 37, 21] = float("inf")
    with torch.no_grad():
        _, ref = oracle_forward("msbd", comp, w, x, q)
    try:
        with torch.no_grad():
            outs = build(eng, "msbd", comp, w)(x.float().cuda(), q.float().cuda())
        torch.cuda.synchronize()
    finally:
        eng.set_stream(0)
    assert outputs_detect("inf pixel", outs, ref), "the oracle's outputs are finite: the plant tests nothing"


def test_joint_step_nan_in_the_qt_stem_reaches_the_mtt_loss(eng):
    from pmp_vvc_tip2023_amd import train_loss
    comp = "Chroma"
    wq = net_weights("q", comp)
    stem = [k for k in sorted(wq) if k.startswith("conv_q1") and k.endswith("weight")][0]
    x, _ = net_inputs(comp)
    _, msbt, msdire = labels()
    qn, bd = build(eng, "q", comp, planted(wq, stem)), build(eng, "msbd", comp, net_weights("msbd", comp))
    try:
        with torch.no_grad():
            xd = x.float().cuda()
            loss = train_loss.loss_func_MSBD(eng, *bd(xd, qn(xd)), msbt, msdire, False, QP[comp])
        torch.cuda.synchronize()
    finally:
        eng.set_stream(0)
    assert not np.isfinite(float(loss)), float(loss)
