"""Time one ResidualBlock, forward + backward, on the library's kernels (pmp_resblock_forward_device / _backward_device through
pmp_vvc_tip2023_amd.resblock) next to eager torch autograd on the same block, and write profiles/resblock_grad.txt.

    python tools/resblock_grad_bench.py [--n 200] [--shapes "32,64,5,64;64,64,3,64;64,64,3,32;64,32,3,32"] [--iters 20] [--warmup 3] [--out FILE]

--shapes: cin,cout,k,size per block, ';'-separated; the default is the nets' 64x64 and 32x32 blocks.  Both sides start from the same
device tensors (x requires a gradient, as every block behind the first does) and end with out, x.grad and the weights' .grad on the
device.  The eager side is the reference's module written out (two bias-free convolutions, ReLU, identity or 1x1 shortcut).

Before anything is timed the two sides are compared, d = max |ours - eager| / max |eager| per tensor, in a way that does not depend on
which side of zero a pre-activation lands: (a) the forward outputs t and out, which are continuous in every rounding; (b) the library's
backward on EAGER's t and out against eager's gradients - the same ReLU masks on both sides.  Either above --tol stops the tool.
Two float32 forwards differ in the last bits, so a few of the millions of pre-activations next to zero get a different `> 0` on the
two sides; one such element moves g_x by a whole term.  The tool counts those elements and reports the end-to-end distance of the
autograd path, which contains them, without judging it.  (c) For the first --f64-images images g_x of both sides is also measured
against a float64 CPU backward with eager's masks.
Times are hipEvent times around `iters` back-to-back forward + backward calls after `warmup` calls, per call; the library's share of
it per direction is timed the same way on the raw device calls.  The file also records E = max |result - f64| / max |f64| of the
float-valued cases of tests/resblock_cases.py next to torch's CPU float32 ops (what tests/test_gpu_resblock_grad.py bounds by 4).
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

import resblock_cases as K  # noqa: E402
from pmp_vvc_tip2023_amd import engine, resblock  # noqa: E402

DEFAULT = "32,64,5,64;64,64,3,64;64,64,3,32;64,32,3,32"
P = lambda t: None if t is None else t.data_ptr()


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


def one(eng, n, cin, cout, k, size, warmup, iters, tol, f64_images):
    g = torch.Generator(device="cuda").manual_seed(cin * 1000 + cout * 10 + k + size)
    rn = lambda scale, *s: torch.randn(s, generator=g, device="cuda") * scale
    x = rn(1.0, n, cin, size, size).requires_grad_()
    w0, w2 = rn((cin * k * k) ** -0.5, cout, cin, k, k).requires_grad_(), rn((cout * k * k) ** -0.5, cout, cout, k, k).requires_grad_()
    wsc = rn(cin ** -0.5, cout, cin, 1, 1).requires_grad_() if cin != cout else None
    g_out = rn(1.0, n, cout, size, size)
    leaves = [t for t in (x, w0, w2, wsc) if t is not None]
    names = ["g_x", "g_w0", "g_w2", "g_wsc"][:len(leaves)]
    shape = (n, size, size, cin, cout, k)
    kept = {}

    def eager():
        for t in leaves:
            t.grad = None
        t_ = F.relu(F.conv2d(x, w0, padding=k // 2))
        out = F.relu(F.conv2d(t_, w2, padding=k // 2) + (x if wsc is None else F.conv2d(x, wsc)))
        kept["t"] = t_.detach()
        out.backward(g_out)
        return out

    def ours():
        for t in leaves:
            t.grad = None
        out = resblock.residual_block(eng, x, w0, w2, wsc)
        out.backward(g_out)
        return out

    out_e = eager().detach()
    t_e, grads_e = kept["t"].contiguous(), [t.grad.clone() for t in leaves]
    out_a = ours().detach()
    grads_a = [t.grad.clone() for t in leaves]
    torch.cuda.synchronize()
    # the two library calls alone: forward, and backward on EAGER's t and out (the same masks as eager's own backward)
    t_o, out_o = torch.empty_like(t_e), torch.empty_like(out_e)
    gr = [torch.empty_like(t) for t in leaves]
    eng.set_stream(torch.cuda.current_stream().cuda_stream)
    fwd = lambda: eng.resblock_forward_device(shape, P(x), P(w0), P(w2), P(wsc), P(t_o), P(out_o))

    def bwd(t_in=t_e, out_in=out_e):
        eng.resblock_backward_device(shape, P(x), P(t_in), P(out_in), P(w0), P(w2), P(wsc), P(g_out), P(gr[0]), P(gr[1]), P(gr[2]),
                                     P(gr[3]) if wsc is not None else None)

    fwd()
    bwd()
    torch.cuda.synchronize()
    d_fwd = {"t": dist(t_o, t_e), "out": dist(out_o, out_e)}
    d_bwd = {nm: dist(a, b) for nm, a, b in zip(names, gr, grads_e)}
    flips = (int(((t_o > 0) != (t_e > 0)).sum()), int(((out_o > 0) != (out_e > 0)).sum()))
    d_auto = max([dist(out_a, out_e)] + [dist(a, b) for a, b in zip(grads_a, grads_e)])
    head = "(%2d,%2d,%d)@%d^2 n %d" % (cin, cout, k, size, n)
    lines = ["%s  agreement with eager torch: forward t %.1e, out %.1e; backward on eager's t and out: %s" % (
        head, d_fwd["t"], d_fwd["out"], ", ".join("%s %.1e" % kv for kv in d_bwd.items()))]
    lines.append("%s  pre-activations on the other side of zero: %d of %d in t, %d of %d in out; end to end through autograd (contains them): %.1e"
                 % (" " * len(head), flips[0], t_e.numel(), flips[1], out_e.numel(), d_auto))
    if f64_images:
        m = min(f64_images, n)
        cpu = lambda a: a.detach().cpu().numpy()
        r = K.backward(cpu(x[:m]), cpu(t_e[:m]), cpu(out_e[:m]), cpu(w0), cpu(w2), None if wsc is None else cpu(wsc).reshape(cout, cin), cpu(g_out[:m]))
        lines.append("%s  g_x of the first %d images against float64 with eager's masks: E ours %.1e, E eager torch %.1e"
                     % (" " * len(head), m, K.rel_err(gr[0][:m].cpu().numpy(), r["g_x"]), K.rel_err(grads_e[0][:m].cpu().numpy(), r["g_x"])))
    bad = max(list(d_fwd.values()) + list(d_bwd.values()))
    if bad > tol:
        print("\n".join(lines))
        raise SystemExit("kernel and eager torch disagree with the same masks: %.3g" % bad)
    t_f, t_b = timed(fwd, warmup, iters), timed(lambda: bwd(t_o, out_o), warmup, iters)
    t_ours, t_eager = timed(ours, warmup, iters), timed(eager, warmup, iters)
    gflop = 3 * 2.0 * n * size * size * cout * (cin * k * k + cout * k * k + (cin if wsc is not None else 0)) / 1e9
    lines.append("%s  ours fwd+bwd %8.3f ms (library calls: fwd %7.3f, bwd %7.3f; %5.1f TFLOP/s over both)   eager torch %8.3f ms   (eager / ours x%.2f)"
                 % (" " * len(head), t_ours, t_f, t_b, gflop / (t_f + t_b), t_eager, t_eager / t_ours))
    return lines


def float_ratios(eng):
    """E of the kernels and of torch's CPU float32 ops against float64 on the float-valued test cases, per output tensor."""
    lines = []
    up = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda()
    eng.set_stream(torch.cuda.current_stream().cuda_stream)
    for name in K.FLOAT:
        c = K.make_float(name)
        n, h, w, cin, cout, k = c["shape"]
        t64, out64 = K.forward(c["x"], c["w0"], c["w2"], c["wsc"])
        c["t"], c["out"] = K.as_f32(t64), K.as_f32(out64)
        ref = dict(K.backward(c["x"], c["t"], c["out"], c["w0"], c["w2"], c["wsc"], c["g_out"]), t=t64, out=out64)
        t32, out32 = K.forward(c["x"], c["w0"], c["w2"], c["wsc"], torch.float32)
        cpu = dict(K.backward(c["x"], c["t"], c["out"], c["w0"], c["w2"], c["wsc"], c["g_out"], torch.float32), t=t32, out=out32)
        d = {key: up(c[key]) for key in ("x", "t", "out", "w0", "w2", "wsc", "g_out")}
        o = {key: torch.empty(ref[key].shape, device="cuda") for key in K.OUTPUTS if ref[key] is not None}
        eng.resblock_forward_device(c["shape"], P(d["x"]), P(d["w0"]), P(d["w2"]), P(d["wsc"]), P(o["t"]), P(o["out"]))
        eng.resblock_backward_device(c["shape"], P(d["x"]), P(d["t"]), P(d["out"]), P(d["w0"]), P(d["w2"]), P(d["wsc"]), P(d["g_out"]), P(o["g_x"]),
                                     P(o["g_w0"]), P(o["g_w2"]), P(o.get("g_wsc")))
        torch.cuda.synchronize()
        for key in K.OUTPUTS:
            if ref[key] is not None:
                mine, theirs = K.rel_err(o[key].cpu().numpy(), ref[key]), K.rel_err(cpu[key], ref[key])
                lines.append("%-9s %-24s %-5s E kernel %.2e   E torch CPU float32 %.2e   ratio %.2f" % (name, c["shape"], key, mine, theirs, mine / theirs))
    return lines


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--n", default=200, type=int, help="blocks per batch (200 is the reference's batch size)")
    ap.add_argument("--shapes", default=DEFAULT)
    ap.add_argument("--iters", default=20, type=int)
    ap.add_argument("--warmup", default=3, type=int)
    ap.add_argument("--tol", default=1e-4, type=float, help="largest accepted distance to eager torch with the same ReLU masks")
    ap.add_argument("--f64-images", default=2, type=int, help="images whose g_x is also measured against float64 on the CPU (0 = none)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "resblock_grad.txt"), help="the file the lines are written to")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("resblock_grad_bench: no GPU - there is no CPU fallback")
    eng = engine.Engine(0)
    lines = ["one ResidualBlock forward + backward (x, w0, w2, wsc gradients), this library against eager torch-ROCm autograd, float32, hipEvents, "
             "%d calls after %d warm-up calls, %s" % (a.iters, a.warmup, torch.cuda.get_device_name(0)), ""]
    with torch.cuda.stream(torch.cuda.Stream()):        # a real stream: the library adopts it, and the events time what runs on it
        for spec in a.shapes.split(";"):
            cin, cout, k, size = (int(v) for v in spec.split(","))
            got = one(eng, a.n, cin, cout, k, size, a.warmup, a.iters, a.tol, a.f64_images)
            print("\n".join(got), flush=True)
            lines += got
        lines += ["", "float-valued test cases, E = max |result - f64| / max |f64| per tensor (tests/test_gpu_resblock_grad.py bounds the ratio by 4):"]
        got = float_ratios(eng)
        print("\n".join(got), flush=True)
        lines += got
    eng.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
