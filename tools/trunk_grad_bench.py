"""Time a trunk of ResidualBlocks (with its pool), forward + backward, three ways, and write profiles/trunk_grad.txt:
  (a) the trunk call: pmp_trunk_forward_device / _backward_device through pmp_vvc_tip2023_amd.trunk - activations blocked throughout;
  (b) the same trunk as a chain of resblock.residual_block calls (pmp_resblock_*_device, dense tensors between the blocks) plus
      F.max_pool2d;
  (c) eager torch-ROCm autograd on the same ops.

    python tools/trunk_grad_bench.py [--n 200] [--trunks "M1,M2,B3,Att2"] [--iters 10] [--warmup 2] [--trunk-only] [--out FILE]

Trunks (Model_QBD.py:112-125): M1 = 32->64 k5, 5 x 64->64 k3, pool, at 64^2;  M2 = 4 x 64->64 k3, pool, at 32^2;
B3 = 64->32->16->8 k3, pool, at 32^2;  Att2 = 3->32->64 k3, no pool, at 32^2.
All three start from the same device tensors (x requires a gradient) and end with y, x.grad and the weights' .grad on the device.
Per trunk the order of measurement is chain / trunk / chain / eager, so the spread between the two chain runs stands next to the
difference it is compared with.  Times are hipEvent times around `iters` back-to-back forward + backward calls after `warmup` calls.

Agreement, before anything is timed: (a) against (b) must be bit for bit (the same kernels on the same values in the same order);
(a) against (c) is reported as d = max |a - c| / max |c| per tensor - two float32 forwards differ in their last bits, a few
pre-activations next to zero get a different `> 0`, and one such element moves a gradient by a whole term, so this is not judged.
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from pmp_vvc_tip2023_amd import engine, resblock, trunk  # noqa: E402

# name -> (size, cin, [(cout, k), ...], pool)
TRUNKS = {
    "M1": (64, 32, [(64, 5)] + [(64, 3)] * 5, True),
    "M2": (32, 64, [(64, 3)] * 4, True),
    "B3": (32, 64, [(32, 3), (16, 3), (8, 3)], True),
    "Att2": (32, 3, [(32, 3), (64, 3)], False),
}


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


def one(eng, name, n, warmup, iters, trunk_only=False):
    size, cin, blocks, pool = TRUNKS[name]
    g = torch.Generator(device="cuda").manual_seed(1000 + sum(ord(ch) for ch in name))
    rn = lambda scale, *s: torch.randn(s, generator=g, device="cuda") * scale
    x = rn(1.0, n, cin, size, size).requires_grad_()
    ws, ci = [], cin
    for co, k in blocks:
        ws.append((rn((ci * k * k) ** -0.5, co, ci, k, k).requires_grad_(), rn((co * k * k) ** -0.5, co, co, k, k).requires_grad_(),
                   rn(ci ** -0.5, co, ci, 1, 1).requires_grad_() if ci != co else None))
        ci = co
    so = size // 2 if pool else size
    g_y = rn(1.0, n, ci, so, so)
    leaves = [x] + [w for blk in ws for w in blk if w is not None]

    def finish(y):
        y = F.max_pool2d(y, 2) if pool else y
        y.backward(g_y)
        return y

    def clear():
        for t in leaves:
            t.grad = None

    def ours():
        clear()
        y = trunk.trunk(eng, x, ws, pool=pool)
        y.backward(g_y)
        return y

    def chain():
        clear()
        a = x
        for w0, w2, wsc in ws:
            a = resblock.residual_block(eng, a, w0, w2, wsc)
        return finish(a)

    def eager():
        clear()
        a = x
        for w0, w2, wsc in ws:
            k = w0.shape[2]
            t = F.relu(F.conv2d(a, w0, padding=k // 2))
            a = F.relu(F.conv2d(t, w2, padding=k // 2) + (a if wsc is None else F.conv2d(a, wsc)))
        return finish(a)

    if trunk_only:                                      # under a profiler: nothing but the trunk call's launches
        return ["%s  trunk call alone: %.3f ms" % (name, timed(ours, warmup, iters))]
    res = {}
    for what, fn in (("trunk", ours), ("chain", chain), ("eager", eager)):
        y = fn().detach()
        res[what] = [y] + [t.grad.clone() for t in leaves]
    torch.cuda.synchronize()
    same = all(torch.equal(a, b) for a, b in zip(res["trunk"], res["chain"]))
    d_eager = [dist(a, b) for a, b in zip(res["trunk"], res["eager"])]
    shape = (n, size, size, cin, blocks, 1 if pool else 0)
    head = "trunk_%-4s %d blocks%s at %d^2, n %d" % (name, len(blocks), " + pool" if pool else "", size, n)
    lines = ["%s  saved activations (pmp_trunk_saved_bytes): %.1f MB" % (head, engine.Engine.trunk_saved_bytes(shape) / 1e6),
             "%s  trunk call against the chain of block calls: %s;  against eager torch: d(y) %.1e, d(g_x) %.1e, worst weight gradient %.1e"
             % (" " * len(head), "bit for bit" if same else "DIFFERENT", d_eager[0], d_eager[1], max(d_eager[2:]))]
    del res
    if not same:
        print("\n".join(lines))
        raise SystemExit("the trunk call and the chain of block calls disagree")
    t_c1 = timed(chain, warmup, iters)
    t_a = timed(ours, warmup, iters)
    t_c2 = timed(chain, warmup, iters)
    t_e = timed(eager, warmup, iters)
    t_c = min(t_c1, t_c2)
    lines.append("%s  fwd+bwd ms: chain %8.3f | trunk %8.3f | chain %8.3f | eager torch %8.3f    trunk against chain x%.2f (chain runs apart by %.1f %%), "
                 "against eager x%.2f" % (" " * len(head), t_c1, t_a, t_c2, t_e, t_c / t_a, 100 * abs(t_c1 - t_c2) / t_c, t_e / t_a))
    return lines


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--n", default=200, type=int, help="blocks per batch (200 is the reference's batch size)")
    ap.add_argument("--trunks", default="M1,M2,B3,Att2")
    ap.add_argument("--iters", default=10, type=int)
    ap.add_argument("--warmup", default=2, type=int)
    ap.add_argument("--trunk-only", action="store_true", help="run the trunk call alone, nothing compared (for a kernel trace of its launches)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "trunk_grad.txt"), help="the file the lines are written to")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("trunk_grad_bench: no GPU - there is no CPU fallback")
    eng = engine.Engine(0)
    lines = ["a trunk of ResidualBlocks forward + backward (x and every weight's gradient): the trunk call (activations blocked throughout) against "
             "the chain of block calls + F.max_pool2d and against eager torch-ROCm autograd, float32, hipEvents, %d calls after %d warm-up calls, %s"
             % (a.iters, a.warmup, torch.cuda.get_device_name(0)), ""]
    with torch.cuda.stream(torch.cuda.Stream()):        # a real stream: the library adopts it, and the events time what runs on it
        for name in a.trunks.split(","):
            got = one(eng, name, a.n, a.warmup, a.iters, a.trunk_only)
            print("\n".join(got), flush=True)
            lines += got
            torch.cuda.empty_cache()
    eng.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
