"""GPU: pmp_adam_step_device and optim.Adam (include/pmp.h, TRAINING STEP) against torch.optim.Adam(foreach=False) on the CPU.

The bound (adam_cases.check_bound): per tensor, each of param, m and v within four times the distance of torch's CPU float32 run
from the float64 restatement - the project's yardstick for the training calls (test_gpu_q_net.py) - and never tighter than one
float32 ulp of that tensor's largest magnitude over the run (adam_cases.peaks says why it is not the final values' alone), because
torch's own distance can be a fraction of an ulp on a short tensor.  On the CPU (test_adam_cases_cpu.py) the header's order of
operations, restated in numpy, lies a quarter of the bound away at worst.
Tensor lists: the sizes 1 .. 204 800 in one call, aligned to 16 bytes and 4 bytes behind (both paths of the kernel); the 92 shapes of
the luma joint step in one call; 300 one-element tensors, which cross the argument block's table.  Steps 1, 2, 3 from a zero state and
step 1000 from a given state; gradient scales 1e-3, 1 and 1e3 and a gradient with exact zeros."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import adam_cases as A
import train_rig as R

pytestmark = pytest.mark.gpu
eng = R.engine_fixture()
KEYS = ("param", "grad", "m", "v")


@functools.lru_cache(maxsize=None)
def case(name, scale, state, zeros=False):
    """-> (tensors, steps, first step, torch's CPU float32 results, the float64 restatement's, its peaks), computed once"""
    torch.set_num_threads(16)
    t = A.tensors(A.lists()[name], 20 + len(name), scale, zeros=zeros, state=state)
    steps, first = (1, 1000) if state else (3, 1)
    return t, steps, first, A.torch_adam(t, steps, torch.float32, first)[0], A.run(A.adam64, t, steps, first), A.peaks(t, steps, first)


class AdamDev:
    """A call's tensors on the device, each in a NaN-guarded allocation of its own: 4 bytes behind a 16-byte boundary (off4) or on one."""

    def __init__(self, t, off4=True):
        self.g = {k: [R.Off4(R.up(a)) for a in t[k]] for k in KEYS}
        self.d = {k: [g.view if off4 else g.view.clone() for g in self.g[k]] for k in KEYS}
        self.counts = [a.size for a in t["param"]]
        R.torch_done()

    def ptrs(self, k):
        return [R.P(a) for a in self.d[k]]

    def step(self, e, step, **hyper):
        e.adam_step_device(self.ptrs("param"), self.ptrs("grad"), self.ptrs("m"), self.ptrs("v"), self.counts, step, **hyper)

    def results(self, e):
        e.synchronize()
        assert all(g.guards_intact() for k in KEYS for g in self.g[k])
        return {k: [R.num(a).ravel() for a in self.d[k]] for k in ("param", "m", "v")}

    def untouched(self, t, keys=KEYS):
        return all(R.same_bits(R.num(a).ravel(), src) for k in keys for a, src in zip(self.d[k], t[k]))


def run_case(e, c, off4=True):
    t, steps, first = c[:3]
    d = AdamDev(t, off4)
    for i in range(steps):
        d.step(e, first + i)
    got = d.results(e)
    assert d.untouched(t, ("grad",)), "a gradient changed"
    return got


@pytest.mark.parametrize("off4", [True, False], ids=["off4", "aligned"])
@pytest.mark.parametrize("state", [False, True], ids=["steps1to3", "step1000"])
@pytest.mark.parametrize("scale", A.SCALES)
def test_sizes_in_one_call_within_four_times_torch(eng, scale, state, off4):
    c = case("sizes", scale, state, zeros=scale == 1.0)
    print("worst distance / bound: %.3f" % A.check_bound("sizes", run_case(eng, c, off4), c[3], c[4], c[5]))


@pytest.mark.parametrize("state", [False, True], ids=["steps1to3", "step1000"])
def test_the_92_tensors_of_the_luma_joint_step_in_one_call(eng, state):
    from pmp_vvc_tip2023_amd import _lib
    c = case("joint", 1.0, state)
    assert len(c[0]["param"]) == 92 <= _lib.PMP_ADAM_TABLE
    print("worst distance / bound: %.3f" % A.check_bound("joint", run_case(eng, c), c[3], c[4], c[5]))


def test_300_one_element_tensors_cross_the_table(eng):
    from pmp_vvc_tip2023_amd import _lib
    c = case("ones", 1.0, False)
    assert len(c[0]["param"]) > 3 * _lib.PMP_ADAM_TABLE
    print("worst distance / bound: %.3f" % A.check_bound("ones", run_case(eng, c), c[3], c[4], c[5]))


def test_nonfinite_gradients_travel_as_in_torch(eng):
    t = A.nonfinite_case()
    t32, _ = A.torch_adam(t, 1, torch.float32, 5)
    d = AdamDev(t)
    d.step(eng, 5)
    got = d.results(eng)
    for k in got:
        assert np.array_equal(A.pattern(got[k][0]), A.pattern(t32[k][0])), k
    fin = A.pattern(t32["param"][0]) == 0
    r64 = A.run(A.adam64, t, 1, 5)
    part = lambda r: {k: [r[k][0][fin]] for k in r}
    start = {k: [np.abs(t[k][0][fin]).max()] for k in r64}
    A.check_bound("finite elements beside the others", part(got), part(t32), part(r64),
                  {k: [max(start[k][0], np.abs(r64[k][0][fin]).max())] for k in r64})


def test_tensors_outside_the_call_are_untouched(eng):
    t = A.tensors([3, 65, 1025], 8)
    d = AdamDev(t)
    rest = A.tensors([3, 65, 1025], 9)
    by = AdamDev(rest)
    d.step(eng, 1)
    d.results(eng)
    by.results(eng)
    assert by.untouched(rest)


def test_same_bits_on_every_run_stream_and_context(eng):
    R.same_bits_on_every_run_stream_and_context(
        eng, lambda e, c: {"%s%d" % (k, i): a for k, v in run_case(e, c).items() for i, a in enumerate(v)}, case("sizes", 1.0, True))


def test_refusals_leave_all_four_arrays_untouched(eng):
    from pmp_vvc_tip2023_amd import _lib
    t = A.tensors([5, 64, 257], 12, state=True)
    d = AdamDev(t)
    nt = len(d.counts)
    nan, inf = float("nan"), float("inf")

    def call(nm, which, ntensors=nt, null=(), entry=None, counts=None, step=1, lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8):
        ps = {k: d.ptrs(k) for k in KEYS}
        for k, i, v in entry or ():
            ps[k][i] = v
        arr = {k: None if k in null else _lib.pointer_array(ps[k], nt) for k in KEYS}
        cnt = None if "count" in null else (C.c_int64 * nt)(*(counts or d.counts))
        p = None if "p" in null else C.byref(_lib.AdamParams(lr, beta1, beta2, eps))
        return eng.lib.pmp_adam_step_device(eng.h, p, ntensors, arr["param"], arr["grad"], arr["m"], arr["v"], cnt, step)

    P0 = d.ptrs("param")[0]
    tries = [("ntensors 0", "", "", dict(ntensors=0)), ("ntensors -1", "", "", dict(ntensors=-1)), ("null params", "", "", dict(null=("p",))),
             ("null count", "", "", dict(null=("count",)))] + \
            [("null array " + k, "", "", dict(null=(k,))) for k in KEYS] + \
            [("null entry " + k, "", "", dict(entry=[(k, 1, None)])) for k in KEYS] + \
            [("count 0", "", "", dict(counts=[5, 0, 257])), ("count -3", "", "", dict(counts=[5, 64, -3])), ("step 0", "", "", dict(step=0)),
             ("step -1", "", "", dict(step=-1)), ("lr nan", "", "", dict(lr=nan)), ("lr inf", "", "", dict(lr=inf)), ("beta1 nan", "", "", dict(beta1=nan)),
             ("beta2 inf", "", "", dict(beta2=inf)), ("eps nan", "", "", dict(eps=nan)), ("beta1 1", "", "", dict(beta1=1.0)),
             ("beta1 negative", "", "", dict(beta1=-0.1)), ("beta2 1", "", "", dict(beta2=1.0)), ("beta2 negative", "", "", dict(beta2=-1e-9)),
             ("eps 0", "", "", dict(eps=0.0)), ("eps negative", "", "", dict(eps=-1e-8)),
             ("m over a param", "", "", dict(entry=[("m", 1, P0)])), ("a grad inside another param", "", "", dict(entry=[("grad", 2, P0 + 8)])),
             ("the same param twice", "", "", dict(entry=[("param", 1, P0)], counts=[5, 5, 257])),
             ("a tensor two bytes off", "", "", dict(entry=[("v", 0, d.ptrs("v")[0] + 2)]))]
    R.refuse_all(eng, tries, call)
    assert d.untouched(t) and all(g.guards_intact() for k in KEYS for g in d.g[k])
    assert call("", "") == 0                                  # the same call, unharmed, is accepted
    d.results(eng)
    assert not d.untouched(t, ("param", "m", "v"))


# ---- the optimiser class
def test_state_dict_goes_to_torchs_adam_and_back_and_the_next_steps_agree(eng):
    from pmp_vvc_tip2023_amd import optim
    t = A.tensors([1, 5, 64, 1025], 31)
    grads = [A.tensors([1, 5, 64, 1025], 32 + i)["grad"] for i in range(3)]
    ps = [torch.nn.Parameter(R.up(a)) for a in t["param"]]
    opt = optim.Adam(eng, ps, lr=2e-3, betas=(0.8, 0.99), eps=1e-7)
    hyper = dict(lr=2e-3, betas=(0.8, 0.99), eps=1e-7)
    try:
        for i in range(2):
            for p, g in zip(ps, grads[i]):
                p.grad = R.up(g)
            opt.step()
        torch.cuda.synchronize()
        sd = opt.state_dict()
        assert sorted(sd["state"][0]) == ["exp_avg", "exp_avg_sq", "step"] and float(sd["state"][0]["step"]) == 2.0
        # into torch's optimiser on the CPU, on the parameters as they are now
        now = {"param": [R.num(p.detach()).ravel() for p in ps], "m": [R.num(opt.state[p]["exp_avg"]).ravel() for p in ps],
               "v": [R.num(opt.state[p]["exp_avg_sq"]).ravel() for p in ps]}
        cps = [torch.nn.Parameter(torch.from_numpy(a.copy())) for a in now["param"]]
        topt = torch.optim.Adam(cps, foreach=False)
        topt.load_state_dict(sd)
        g0 = topt.param_groups[0]
        assert (g0["lr"], tuple(g0["betas"]), g0["eps"]) == (2e-3, (0.8, 0.99), 1e-7)
        for p, a in zip(cps, now["m"]):
            assert topt.state[p]["exp_avg"].device.type == "cpu" and R.same_bits(topt.state[p]["exp_avg"].numpy(), a)
        # one more step in each
        for p, cp, g in zip(ps, cps, grads[2]):
            p.grad, cp.grad = R.up(g), torch.from_numpy(g.copy())
        opt.step()
        topt.step()
        torch.cuda.synchronize()
        got = {"param": [R.num(p.detach()).ravel() for p in ps], "m": [R.num(opt.state[p]["exp_avg"]).ravel() for p in ps],
               "v": [R.num(opt.state[p]["exp_avg_sq"]).ravel() for p in ps]}
        t32 = {"param": [p.detach().numpy() for p in cps], "m": [topt.state[p]["exp_avg"].numpy() for p in cps],
               "v": [topt.state[p]["exp_avg_sq"].numpy() for p in cps]}
        r64 = A.run(A.adam64, dict(now, grad=grads[2]), 1, 3, **hyper)
        print("worst distance / bound: %.3f" % A.check_bound("third step", got, t32, r64, A.peaks(dict(now, grad=grads[2]), 1, 3, **hyper)))
        # and back: torch's state into a fresh optimiser of ours
        ps2 = [torch.nn.Parameter(R.up(a)) for a in t32["param"]]
        opt2 = optim.Adam(eng, ps2)
        opt2.load_state_dict(topt.state_dict())
        assert opt2.param_groups[0]["lr"] == 2e-3 and float(opt2.state[ps2[0]]["step"]) == 3.0
        for p, a in zip(ps2, t32["v"]):
            assert opt2.state[p]["exp_avg_sq"].is_cuda and R.same_bits(R.num(opt2.state[p]["exp_avg_sq"]), a)
        ps2[1].grad = R.up(grads[0][1])                      # the others have no .grad: skipped, as torch skips them
        opt2.step()
        torch.cuda.synchronize()
        assert [float(opt2.state[p]["step"]) for p in ps2] == [3.0, 4.0, 3.0, 3.0]
        assert not R.same_bits(R.num(ps2[1].detach()), t32["param"][1]) and R.same_bits(R.num(ps2[2].detach()), t32["param"][2])
    finally:
        eng.set_stream(0)


def test_one_step_of_both_nets_changes_every_parameter(eng):
    """test_gpu_q_net.test_one_adam_step_of_both_nets_changes_every_parameter with optim.Adam in torch's place"""
    import test_gpu_q_net as Q
    from pmp_vvc_tip2023_amd import optim, train_loss
    comp = "Chroma"
    x, _ = Q.inputs(comp, 1)
    g = torch.Generator().manual_seed(77)
    qt8 = torch.randint(0, 4, (1, 8, 8), generator=g).to(torch.uint8).cuda()
    msbt = torch.randint(0, 4, (1, 3, 16, 16), generator=g).to(torch.uint8).cuda()
    msdire = (torch.randint(0, 3, (1, 3, 16, 16), generator=g) - 1).to(torch.int8).cuda()
    net, bd = Q.qnet(eng, comp), Q.mtt(eng, comp)
    both = dict([("q." + k, v) for k, v in net.named_parameters()] + [("bd." + k, v) for k, v in bd.named_parameters()])
    before = {k: v.detach().clone() for k, v in both.items()}
    opt = optim.Adam(eng, list(net.parameters()) + list(bd.parameters()), lr=1e-4)
    try:
        xd = x.float().cuda()
        q = net(xd)
        out0, out1, out2 = bd(xd, q)
        loss = train_loss.loss_func_QBD(eng, q, out0, out1, out2, qt8, msbt, msdire, False, Q.NETS[comp])
        loss.backward()
        opt.step()
        torch.cuda.synchronize()
    finally:
        eng.set_stream(0)
    assert len(before) == 20 + 72 and np.isfinite(float(loss.detach()))
    for k, v in both.items():
        assert v.grad is not None and torch.isfinite(v.grad).all() and not torch.equal(v.detach(), before[k]), k
        assert torch.isfinite(v.detach()).all(), k
