"""Time a QT net's tail in training two ways, and whole steps through this library, and write profiles/qtail_grad.txt:
  (a) the tail call, pmp_qtail_*_device through pmp_vvc_tip2023_amd.qtail, forward + backward, next to
  (b) eager torch-ROCm autograd on the reference's statements (Model_QBD.py:83-90) on the same tensors: conv2d, relu, max_pool2d,
      interpolate, cat - in the order eager / this library / eager;
  (c) one whole QNet step, and one whole joint step QNet + MSBDNet + train_loss.loss_func_QBD (train_QBD), through this library ALONE.
The whole nets are NOT compared with eager torch: the one run that did so for an MTT net at n = 200 ended in a GPU memory fault whose
cause was not found.  A torch.cuda.synchronize() stands between every two legs.

    python tools/qtail_grad_bench.py [--n 200] [--iters 10] [--warmup 2] [--nets "Luma,Chroma"] [--out FILE]

Times are hipEvent times around `iters` back-to-back forward + backward calls after `warmup` calls.  No ratio is judged; a line where
this library is slower than eager torch is marked SLOWER.  Agreement is reported as d = max |a - b| / max |b| over the output and the
gradients, not judged either (tests/test_gpu_qtail_grad.py and test_gpu_q_net.py hold the calls against float64).
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from pmp_vvc_tip2023_amd import engine, msbd_net, q_net, qtail, train_loss  # noqa: E402


def timed(fn, warmup, iters):
    for _ in range(warmup):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters            # milliseconds per call


def dist(a, b):
    return float((a - b).abs().max() / b.abs().max())


def tail(eng, n, warmup, iters):
    g = torch.Generator(device="cuda").manual_seed(5100)
    rn = lambda scale, *s: torch.randn(s, generator=g, device="cuda") * scale
    leaf = lambda scale, *s: rn(scale, *s).requires_grad_()
    x4, g_x9 = leaf(1.0, n, 64, 16, 16), rn(1.0, n, 8, 8, 8)
    blocks = [(leaf((9 * ci) ** -0.5, co, ci, 3, 3), leaf((9 * co) ** -0.5, co, co, 3, 3), leaf(ci ** -0.5, co, ci, 1, 1) if ci != co else None)
              for co, ci in qtail.CHANNELS]
    leaves = [x4] + [t for b in blocks for t in b if t is not None]

    def rb(x, w0, w2, wsc):
        t = F.relu(F.conv2d(x, w0, padding=1))
        return F.relu(F.conv2d(t, w2, padding=1) + (x if wsc is None else F.conv2d(x, wsc)))

    def eager():
        x5 = rb(x4, *blocks[0])
        x6 = torch.cat([x5] + [F.interpolate(F.max_pool2d(x5, s), scale_factor=s) for s in (2, 4, 8)], 1)
        return rb(F.max_pool2d(rb(rb(x6, *blocks[1]), *blocks[2]), 2), *blocks[3])

    def run(fn):
        for t in leaves:
            t.grad = None
        x9 = fn()
        x9.backward(g_x9)
        return x9

    res = {}
    for what, fn in (("ours", lambda: qtail.qtail(eng, x4, blocks)), ("eager", eager)):
        x9 = run(fn).detach().clone()
        res[what] = [x9] + [t.grad.clone() for t in leaves]
        torch.cuda.synchronize()
    d = max(dist(a, b) for a, b in zip(res["ours"], res["eager"]))
    del res
    t_e1 = timed(lambda: run(eager), warmup, iters)
    torch.cuda.synchronize()
    t_a = timed(lambda: run(lambda: qtail.qtail(eng, x4, blocks)), warmup, iters)
    torch.cuda.synchronize()
    t_e2 = timed(lambda: run(eager), warmup, iters)
    torch.cuda.synchronize()
    t_e = min(t_e1, t_e2)
    return "%-44s fwd+bwd ms: eager torch %9.3f | this library %9.3f | eager torch %9.3f    against eager x%.2f%s (eager runs apart by %.1f %%);  " \
           "worst d %.1e" % ("QT tail (resblock_q3 .. q6), n %d, 16x16" % n, t_e1, t_a, t_e2, t_e / t_a, "  SLOWER" if t_a > t_e else "",
                             100 * abs(t_e1 - t_e2) / t_e, d)


def whole(eng, comp, n, warmup, iters):
    """-> two lines: a QNet step on sum(q * g), and a joint QNet + MSBDNet step on loss_func_QBD."""
    luma = comp == "Luma"
    torch.manual_seed(5200 + luma)
    net, bd = q_net.QNet(eng, luma).cuda(), msbd_net.MSBDNet(eng, luma).cuda()
    g = torch.Generator(device="cuda").manual_seed(5300 + luma)
    x = torch.randint(0, 256, (n, 1, 68, 68) if luma else (n, 3, 34, 34), generator=g, device="cuda").float() / 255
    g_q = torch.randn((n, 1, 8, 8), generator=g, device="cuda")
    qt8 = torch.randint(0, 4, (n, 8, 8), generator=g, device="cuda").to(torch.uint8)
    msbt = torch.randint(0, 4, (n, 3, 16, 16), generator=g, device="cuda").to(torch.uint8)
    msdire = (torch.randint(0, 3, (n, 3, 16, 16), generator=g, device="cuda") - 1).to(torch.int8)
    params = list(net.parameters()) + list(bd.parameters())

    def clear():
        for t in params:
            t.grad = None

    def alone():
        clear()
        (net(x) * g_q).sum().backward()

    def joint():
        clear()
        q = net(x)
        train_loss.loss_func_QBD(eng, q, *bd(x, q), qt8, msbt, msdire, luma, 22).backward()

    lines = []
    for label, fn, ps in (("%s_Q_Net step, n %d (20 parameters)" % (comp, n), alone, list(net.parameters())),
                          ("%s train_QBD step: Q + MSBD nets + loss, n %d" % (comp, n), joint, params)):
        fn()
        torch.cuda.synchronize()
        assert all(t.grad is not None and bool(torch.isfinite(t.grad).all()) for t in ps)
        lines.append("%-44s fwd+bwd ms: this library %9.3f" % (label, timed(fn, warmup, iters)))
        torch.cuda.synchronize()
    return lines


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--n", default=200, type=int, help="blocks per batch (200 is the reference's batch size)")
    ap.add_argument("--nets", default="Luma,Chroma")
    ap.add_argument("--iters", default=10, type=int)
    ap.add_argument("--warmup", default=2, type=int)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "qtail_grad.txt"), help="the file the lines are written to")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("qtail_grad_bench: no GPU - there is no CPU fallback")
    eng = engine.Engine(0)
    lines = ["a QT net's tail, one whole QT net step and one joint train_QBD step, forward + backward: this library (the tail also against "
             "eager torch-ROCm autograd), float32, hipEvents, %d calls after %d warm-up calls, %s" % (a.iters, a.warmup, torch.cuda.get_device_name(0)), ""]
    with torch.cuda.stream(torch.cuda.Stream()):        # a real stream: the library adopts it, and the events time what runs on it
        got = [tail(eng, a.n, a.warmup, a.iters)]
        for comp in [c for c in a.nets.split(",") if c]:
            torch.cuda.synchronize()
            torch.cuda.empty_cache()
            got += whole(eng, comp, a.n, a.warmup, a.iters)
        print("\n".join(got), flush=True)
        lines += got
    eng.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
