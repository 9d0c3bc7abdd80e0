"""Time the joints of an MTT net's training step - head, attention input and gate - two ways, and one whole step of the net through
this library, and write profiles/head_grad.txt:
  (a) this library: pmp_head_*_device / pmp_gate_*_device through pmp_vvc_tip2023_amd.head, and msbd_net.MSBDNet;
  (b) for the joints, eager torch-ROCm autograd on the reference's statements (Model_QBD.py:139-153): conv2d with bias, the in-place
      carry, F.interpolate, torch.cat, the product.
The whole net is NOT compared with eager torch here: the one run that did so at n = 200 ended in a GPU memory fault whose cause was
not found, and that leg was taken out.

    python tools/head_grad_bench.py [--n 200] [--iters 10] [--warmup 2] [--nets "Luma,Chroma"] [--out FILE]

Joints, at the nets' sizes (the heads work at 16x16 in both nets):
  B1   out0 = conv_B1(x6); out0q = cat[up2(x1), out0];                 xb1 = x5 * x_att0          (x_att0 a given tensor [n,64,16,16])
  B2   out1 = conv_B2(xb2); out1[:,0] += out0[:,0]; out1q = cat[up4(x1), up2(out1)];  xb3 = x4 * x_att1   (x_att1 [n,64,32,32])
  B3   out2 = conv_B3(xb4); out2[:,0] += out1[:,0]
Both ways start from the same device tensors and end with every output and the .grad of every leaf on the device.  Times are hipEvent
times around `iters` back-to-back forward + backward calls after `warmup` calls, in the order eager / ours / eager.  No ratio is judged:
the joints are well under 1 % of a step; a line where this library is slower than eager torch is marked SLOWER.  Agreement is reported
as d = max |a - b| / max |b| over the outputs and gradients, not judged either (tests/test_gpu_head_grad.py and test_gpu_msbd_net.py
hold the calls against float64).
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from pmp_vvc_tip2023_amd import engine, head, msbd_net  # noqa: E402


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


def compare(label, leaves, ours, eager, warmup, iters):
    """ours() / eager() -> a list of outputs after running backward into the leaves' .grad."""
    def run(fn):
        for t in leaves:
            t.grad = None
        return fn()

    res = {}
    for what, fn in (("ours", ours), ("eager", eager)):
        outs = [o.detach().clone() for o in run(fn)]
        res[what] = outs + [t.grad.clone() for t in leaves]
    torch.cuda.synchronize()
    d = max(dist(a, b) for a, b in zip(res["ours"], res["eager"]))
    del res
    t_e1 = timed(lambda: run(eager), warmup, iters)
    t_a = timed(lambda: run(ours), warmup, iters)
    t_e2 = timed(lambda: run(eager), warmup, iters)
    t_e = min(t_e1, t_e2)
    return "%-34s fwd+bwd ms: eager torch %9.3f | this library %9.3f | eager torch %9.3f    against eager x%.2f%s (eager runs apart by %.1f %%);  " \
           "worst d %.1e" % (label, t_e1, t_a, t_e2, t_e / t_a, "  SLOWER" if t_a > t_e else "", 100 * abs(t_e1 - t_e2) / t_e, d)


def joints(eng, n, warmup, iters):
    g = torch.Generator(device="cuda").manual_seed(4100)
    rn = lambda scale, *s: torch.randn(s, generator=g, device="cuda") * scale
    leaf = lambda scale, *s: rn(scale, *s).requires_grad_()
    q = torch.randint(0, 4, (n, 1, 8, 8), generator=g, device="cuda").float()
    lines = []
    # (name, prev?, up, the gate's resolution or None)
    for name, has_prev, up, gate_hw in (("B1", False, (2, 1), 16), ("B2", True, (4, 2), 32), ("B3", True, (0, 0), None)):
        x, w, b = leaf(1.0, n, 8, 16, 16), leaf(72 ** -0.5, 2, 8, 3, 3), leaf(0.1, 2)
        prev = leaf(1.0, n, 2, 16, 16) if has_prev else None
        leaves = [x, w, b] + ([prev] if has_prev else [])
        g_y = rn(1.0, n, 2, 16, 16)
        g_att = rn(1.0, n, 3, up[1] * 16, up[1] * 16) if up[1] else None
        if gate_hw:
            xm, att_out, g_xb = leaf(1.0, n, 64, gate_hw, gate_hw), leaf(1.0, n, 64, gate_hw, gate_hw), rn(1.0, n, 64, gate_hw, gate_hw)
            leaves += [xm, att_out]

        def finish(y, att, xb):
            loss = (y * g_y).sum()
            if att is not None:
                loss = loss + (att * g_att).sum() + (xb * g_xb).sum()
            loss.backward()
            return [y] + ([att, xb] if att is not None else [])

        def ours():
            out = head.head(eng, x, w, b, prev, q if up[1] else None, up)
            y, att = out if up[1] else (out, None)
            return finish(y, att, head.gate(eng, xm, att_out) if gate_hw else None)

        def eager():
            y = F.conv2d(x, w, b, padding=1)
            if has_prev:
                y[:, 0:1, :, :] = y[:, 0:1, :, :] + prev[:, 0:1, :, :]
            att = None
            if up[1]:
                att = torch.cat([F.interpolate(q, scale_factor=up[0]), F.interpolate(y, scale_factor=up[1]) if up[1] > 1 else y], 1)
            return finish(y, att, xm * att_out if gate_hw else None)

        what = "joint %s, n %d: head%s%s" % (name, n, " + attention input" if up[1] else "", " + gate at %d^2" % gate_hw if gate_hw else "")
        lines.append(compare(what, leaves, ours, eager, warmup, iters))
    return lines


def whole_net(eng, comp, n, warmup, iters):
    luma = comp == "Luma"
    torch.manual_seed(4200 + luma)
    net = msbd_net.MSBDNet(eng, luma).cuda()
    g = torch.Generator(device="cuda").manual_seed(4300 + luma)
    x = torch.randint(0, 256, (n, 1, 68, 68) if luma else (n, 3, 34, 34), generator=g, device="cuda").float() / 255
    x1 = torch.randint(0, 4, (n, 1, 8, 8), generator=g, device="cuda").float()
    gs = [torch.randn((n, 2, 16, 16), generator=g, device="cuda") for _ in range(3)]

    def step():
        outs = net(x, x1)
        sum((o * gg).sum() for o, gg in zip(outs, gs)).backward()
        return list(outs)

    label = "%s_MSBD_Net step, n %d (72 parameters)" % (comp, n)

    def ours():
        for t in net.parameters():
            t.grad = None
        return step()

    ours()
    torch.cuda.synchronize()
    assert all(t.grad is not None and bool(torch.isfinite(t.grad).all()) for t in net.parameters())
    return "%-34s fwd+bwd ms: this library %9.3f" % (label, timed(ours, warmup, iters))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--n", default=200, type=int, help="blocks per batch (200 is the reference's batch size)")
    ap.add_argument("--nets", default="Luma,Chroma")
    ap.add_argument("--iters", default=10, type=int)
    ap.add_argument("--warmup", default=2, type=int)
    ap.add_argument("--joints", default=1, type=int, help="0: skip the joints")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "head_grad.txt"), help="the file the lines are written to")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("head_grad_bench: no GPU - there is no CPU fallback")
    eng = engine.Engine(0)
    lines = ["an MTT net's joints (head, attention input, gate) and one whole training step, forward + backward: this library against eager "
             "torch-ROCm autograd, float32, hipEvents, %d calls after %d warm-up calls, %s" % (a.iters, a.warmup, torch.cuda.get_device_name(0)), ""]
    with torch.cuda.stream(torch.cuda.Stream()):        # a real stream: the library adopts it, and the events time what runs on it
        if a.joints:
            got = joints(eng, a.n, a.warmup, a.iters)
            print("\n".join(got), flush=True)
            lines += got
        for comp in [c for c in a.nets.split(",") if c]:
            torch.cuda.empty_cache()
            got = whole_net(eng, comp, a.n, a.warmup, a.iters)
            print(got, flush=True)
            lines.append(got)
    eng.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
