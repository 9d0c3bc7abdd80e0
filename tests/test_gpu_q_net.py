"""GPU: a whole QT net as one torch module (pmp_vvc_tip2023_amd/q_net.py) - stem, two one-block trunks, the tail call and the head -
alone, and in train_QBD's joint step with an MTT net (msbd_net.MSBDNet), where the gradient reaches the QT net through x1.

Yardstick (test_gpu_msbd_net.py's): oracle.nets_torch.q_forward on float64 tensors that require gradients, under autograd on the CPU,
and the same in float32.  d32 is the largest relative max-norm distance, max |a32 - a64| / max |a64| per tensor, of that float32 run
from float64 - over the output, and over the 20 parameter gradients.  Every output and gradient of QNet must lie within 4 * d32 of
float64 in the same norm (4 is the project's margin for float cases against torch's CPU float32).  Luma (QP 22) and Chroma (QP 27) on
the shipped trained QT weights; the blocks are n = 2 synth.recipe_r_blocks(2, 9200 + qp) through the oracle's luma_input /
chroma_input, the upstream gradient randn with seed 5.  With these inputs all 20 parameter gradients are non-zero in float64
(asserted); d32 is 2.5e-7 / 3.3e-7 over the outputs and 1.3e-5 over the gradients.
The joint step (Chroma, n = 1, trained-like MTT weights): the functional sum(o * g) over q and the three MTT outputs; the QT net's 20
gradients within 4 * d32 of the same composite through q_forward and msbd_forward in float64, d32 that composite's own float32 run."""
import functools

import numpy as np
import pytest
import torch

import conftest  # noqa: F401 - puts tools/ on sys.path
import trained_like
import train_rig as R
from oracle import nets_torch as O

pytestmark = pytest.mark.gpu
eng = R.engine_fixture()
NETS = {"Luma": 22, "Chroma": 27}


def q_weights(comp):
    from pmp_vvc_tip2023_amd import weights as W
    return {k: np.asarray(v, np.float32) for k, v in W.load_net_weights(comp + "_Q", NETS[comp])[0].items()}


def inputs(comp, n):
    """-> (x f64 [n,1,68,68] or [n,3,34,34], [g_q, g_out0, g_out1, g_out2] f64)"""
    from pmp_vvc_tip2023_amd import synth
    y, u, v = synth.recipe_r_blocks(n, 9200 + NETS[comp])
    x = O.luma_input(y) if comp == "Luma" else O.chroma_input(y, u, v)
    g = torch.Generator().manual_seed(5)
    gs = [torch.randn((n, 1, 8, 8), generator=g, dtype=torch.float64)] + [torch.randn((n, 2, 16, 16), generator=g, dtype=torch.float64) for _ in range(3)]
    return x.double(), gs


def dist(a, b):
    return {k: float(np.abs(a[k] - b[k]).max() / np.abs(b[k]).max()) for k in b}


@functools.lru_cache(maxsize=None)
def yardstick(comp, joint):
    """-> (out64, grad64 of the QT net's 20 parameters, d32 over the outputs, d32 over those gradients), in float64 on the CPU."""
    torch.set_num_threads(16)
    luma = comp == "Luma"
    x, gs = inputs(comp, 1 if joint else 2)
    runs = {}
    for dt in (torch.float64, torch.float32):
        w = {k: torch.from_numpy(v).to(dt).requires_grad_() for k, v in q_weights(comp).items()}
        outs = [O.q_forward(w, x.to(dt), luma)]
        if joint:
            wbd = {k: torch.from_numpy(v).to(dt) for k, v in trained_like.msbd_weights(comp, NETS[comp]).items()}
            outs += list(O.msbd_forward(wbd, x.to(dt), outs[0], luma))
        sum((o * g.to(dt)).sum() for o, g in zip(outs, gs)).backward()
        runs[dt] = ({"out%d" % i: o.detach().double().numpy() for i, o in enumerate(outs)}, {k: v.grad.double().numpy() for k, v in w.items()})
    (o64, g64), (o32, g32) = runs[torch.float64], runs[torch.float32]
    assert len(g64) == 20 and all(np.abs(v).max() > 0 for v in g64.values()), "every parameter gets a gradient"
    return o64, g64, max(dist(o32, o64).values()), max(dist(g32, g64).values())


def qnet(eng, comp):
    from pmp_vvc_tip2023_amd import q_net
    net = q_net.QNet(eng, comp == "Luma").cuda()
    net.load_state_dict({k: torch.from_numpy(v) for k, v in q_weights(comp).items()})
    return net


def mtt(eng, comp):
    from pmp_vvc_tip2023_amd import msbd_net
    net = msbd_net.MSBDNet(eng, comp == "Luma").cuda()
    net.load_state_dict({k: torch.from_numpy(v) for k, v in trained_like.msbd_weights(comp, NETS[comp]).items()})
    return net


def check(comp, what, outs, net, ref):
    o64, g64, d_out, d_grad = ref
    print("%s %s: d32 over the outputs %.3g, over the QT net's parameter gradients %.3g" % (comp, what, d_out, d_grad))
    worst = {}
    for i, o in enumerate(outs):
        got, want = o.detach().cpu().double().numpy(), o64["out%d" % i]
        assert got.shape == want.shape
        worst["out%d" % i] = float(np.abs(got - want).max() / np.abs(want).max())
    params = dict(net.named_parameters())
    assert sorted(params) == sorted(g64) and len(params) == 20
    for k, want in g64.items():
        assert params[k].grad is not None and params[k].grad.shape == want.shape, k
        worst[k] = float(np.abs(params[k].grad.cpu().double().numpy() - want).max() / np.abs(want).max())
    w_out = max(v for k, v in worst.items() if k.startswith("out"))
    w_grad, k_grad = max((v, k) for k, v in worst.items() if not k.startswith("out"))
    print("%s %s: largest distance over the outputs %.3g (%.2f d32), over the gradients %.3g (%.2f d32, %s)" %
          (comp, what, w_out, w_out / d_out, w_grad, w_grad / d_grad, k_grad))
    for k, v in worst.items():
        assert v <= 4 * (d_out if k.startswith("out") else d_grad), (comp, what, k, v)


@pytest.mark.parametrize("comp", list(NETS))
def test_state_dict_round_trips_with_the_weight_dict(eng, comp):
    wts = q_weights(comp)
    sd = qnet(eng, comp).state_dict()
    assert len(sd) == 20 and sorted(sd) == sorted(wts) and all(tuple(sd[k].shape) == wts[k].shape for k in wts)
    assert all(R.same_bits(sd[k].cpu().numpy(), wts[k]) for k in wts)


@pytest.mark.parametrize("comp", list(NETS))
def test_output_and_gradients_within_four_times_cpu_float32(eng, comp):
    ref = yardstick(comp, False)
    x, gs = inputs(comp, 2)
    net = qnet(eng, comp)
    try:
        q = net(x.float().cuda())
        assert tuple(q.shape) == (2, 1, 8, 8)
        (q * gs[0].float().cuda()).sum().backward()
        torch.cuda.synchronize()
    finally:
        eng.set_stream(0)
    check(comp, "alone", [q], net, ref)


def test_joint_step_reaches_the_qt_net_through_x1(eng):
    comp = "Chroma"
    ref = yardstick(comp, True)
    x, gs = inputs(comp, 1)
    net, bd = qnet(eng, comp), mtt(eng, comp)
    try:
        xd = x.float().cuda()
        q = net(xd)
        outs = [q] + list(bd(xd, q))
        sum((o * g.float().cuda()).sum() for o, g in zip(outs, gs)).backward()
        torch.cuda.synchronize()
    finally:
        eng.set_stream(0)
    check(comp, "with the MTT net", outs, net, ref)
    assert all(p.grad is not None for p in bd.parameters())


def test_one_adam_step_of_both_nets_changes_every_parameter(eng):
    from pmp_vvc_tip2023_amd import train_loss
    comp = "Chroma"
    x, _ = inputs(comp, 1)
    g = torch.Generator().manual_seed(77)
    qt8 = torch.randint(0, 4, (1, 8, 8), generator=g).to(torch.uint8).cuda()
    msbt = torch.randint(0, 4, (1, 3, 16, 16), generator=g).to(torch.uint8).cuda()
    msdire = (torch.randint(0, 3, (1, 3, 16, 16), generator=g) - 1).to(torch.int8).cuda()
    net, bd = qnet(eng, comp), mtt(eng, comp)
    both = dict([("q." + k, v) for k, v in net.named_parameters()] + [("bd." + k, v) for k, v in bd.named_parameters()])
    before = {k: v.detach().clone() for k, v in both.items()}
    opt = torch.optim.Adam(list(net.parameters()) + list(bd.parameters()), lr=1e-4)
    try:
        xd = x.float().cuda()
        q = net(xd)
        out0, out1, out2 = bd(xd, q)
        loss = train_loss.loss_func_QBD(eng, q, out0, out1, out2, qt8, msbt, msdire, False, NETS[comp])
        loss.backward()
        opt.step()
        torch.cuda.synchronize()
    finally:
        eng.set_stream(0)
    assert len(before) == 20 + 72 and np.isfinite(float(loss.detach()))
    for k, v in both.items():
        assert v.grad is not None and torch.isfinite(v.grad).all() and not torch.equal(v.detach(), before[k]), k
