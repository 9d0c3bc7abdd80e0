"""Time the ends of a training step and the whole step, and write profiles/train_step.txt:
  (a) the batch: pmp_batch_gather_device from a set resident on the GPU as bytes (dataset.DeviceDataset), next to what
      Load_Pre_VP_Dataset's DataLoader does per step - rows of the host-side float32 tensors gathered into pinned memory and copied in;
  (b) the optimiser: optim.Adam.step (one launch) next to torch.optim.Adam.step on the same parameters and gradients, in the order
      torch / this library / torch;
  (c) a whole train_QBD step: train_qbd.Trainer.step on a batch gathered on the device, next to the composition without this work -
      tools/qtail_grad_bench.py's joint step (the nets and the loss through this library, the batch already on the device) and
      torch.optim.Adam.step.
No eager reference net runs here; torch's optimiser is not one.

    python tools/train_step_bench.py [--n 200] [--comp Luma,Chroma] [--blocks 4096] [--iters 20] [--warmup 3] [--out FILE]

Times are hipEvent times around `iters` back-to-back calls (20 * iters for the batch and for Adam, which take microseconds) after
`warmup` calls, a torch.cuda.synchronize() between every two legs;
for the host batches that interval holds the host's gathering too, as a training loop waits for it.  No ratio is judged; a line where
this library is slower is marked SLOWER.
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from pmp_vvc_tip2023_amd import dataset, engine, optim, train_loss, train_qbd  # noqa: E402


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


def against(label, unit, t_a1, t_ours, t_a2, other):
    t_o = min(t_a1, t_a2)
    return "%-52s %s: %s %9.3f | this library %9.3f | %s %9.3f    against %s x%.2f%s (its runs apart by %.1f %%)" % (
        label, unit, other, t_a1, t_ours, other, t_a2, other, t_o / t_ours, "  SLOWER" if t_ours > t_o else "", 100 * abs(t_a1 - t_a2) / t_o)


def bench(eng, comp, n, blocks, warmup, iters):
    luma = comp == "Luma"
    rng = np.random.default_rng(6100 + luma)
    y = rng.integers(0, 256, (blocks, 68, 68), dtype=np.uint8)
    u, v = (rng.integers(0, 256, (blocks, 34, 34), dtype=np.uint8) for _ in range(2))
    files = {"blocks": y if luma else (y, u, v), "qt8": rng.integers(1, 5, (blocks, 8, 8), dtype=np.uint8),
             "msbt": rng.integers(0, 4, (blocks, 3, 16, 16), dtype=np.uint8), "msdire": rng.integers(-1, 2, (blocks, 3, 16, 16)).astype(np.int8),
             "n": blocks}
    train = dataset.DeviceDataset(eng, None, comp, 22, "Train", 2, 0, files=files)
    order = dataset.permutation(blocks, True, 1, 0)
    d_order = order.cuda()
    nb = blocks // n
    at = [0]

    def ours_batch():
        b = at[0] = (at[0] + 1) % nb
        return train.gather(d_order[b * n:(b + 1) * n], n)

    # the loader's host tensors (Metrics.py:78-135) and a step's batch from them: index, pin, copy
    x_h = torch.from_numpy(y).float()[:, None]
    if not luma:
        x_h = torch.cat([torch.nn.functional.max_pool2d(x_h, 2), torch.from_numpy(u).float()[:, None], torch.from_numpy(v).float()[:, None]], 1)
    host = [x_h, torch.from_numpy(files["qt8"] - np.uint8(1)).float()[:, None], torch.from_numpy(files["msbt"]).float(),
            torch.from_numpy(files["msdire"]).float()]

    def host_batch():
        b = at[0] = (at[0] + 1) % nb
        idx = order[b * n:(b + 1) * n]
        return [t[idx].pin_memory().cuda(non_blocking=True) for t in host]

    lines = []
    small = 20 * iters                          # the two short legs: enough calls for a window of tens of milliseconds
    t1 = timed(host_batch, warmup, small); torch.cuda.synchronize()
    t2 = timed(ours_batch, warmup, small); torch.cuda.synchronize()
    t3 = timed(host_batch, warmup, small); torch.cuda.synchronize()
    lines.append(against("%s batch of %d from %d blocks" % (comp, n, blocks), "ms", t1, t2, t3, "host batch"))

    args = train_qbd.build_parser().parse_args(["--predID", "2", "--lr", "1e-4"] + (["--isLuma"] if luma else []))
    torch.manual_seed(6200 + luma)
    trainer = train_qbd.Trainer(eng, args, comp, {}, 0)
    params = [p for net in trainer.nets.values() for p in net.parameters()]
    # Adam alone: on copies of the parameters (hundreds of steps on random gradients would wreck the nets the whole step runs on)
    g = torch.Generator(device="cuda").manual_seed(6300 + luma)
    copies = [torch.nn.Parameter(p.detach().clone()) for p in params]
    for p in copies:
        p.grad = torch.randn(p.shape, generator=g, device="cuda") * 1e-3
    topt, ours = torch.optim.Adam(copies, lr=args.lr), optim.Adam(eng, copies, lr=args.lr)
    t1 = timed(topt.step, warmup, small); torch.cuda.synchronize()
    t2 = timed(ours.step, warmup, small); torch.cuda.synchronize()
    t3 = timed(topt.step, warmup, small); torch.cuda.synchronize()
    lines.append(against("%s Adam step, %d tensors, %d parameters" % (comp, len(params), sum(p.numel() for p in params)), "ms", t1, t2, t3, "torch.optim"))

    del topt, ours, copies
    fixed = train.gather(d_order[:n], n)
    net, bd = trainer.nets["Q"], trainer.nets["MSBD"]
    topt = torch.optim.Adam(params, lr=args.lr)

    def composed():
        x, _, msbt, msdire, qt8 = fixed
        for p in params:
            p.grad = None
        q = net(x)
        train_loss.loss_func_QBD(eng, q, *bd(x, q), qt8, msbt, msdire, luma, 22).backward()
        topt.step()

    def whole():
        trainer.step(ours_batch())

    t1 = timed(composed, warmup, iters); torch.cuda.synchronize()
    t2 = timed(whole, warmup, iters); torch.cuda.synchronize()
    t3 = timed(composed, warmup, iters); torch.cuda.synchronize()
    train.check()
    assert all(bool(torch.isfinite(p).all()) for p in params)
    lines.append(against("%s train_QBD step, n %d: gather + nets + loss + Adam" % (comp, n), "ms", t1, t2, t3, "nets + torch.optim"))
    return lines


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--n", default=200, type=int, help="blocks per batch (200 is the reference's batch size)")
    ap.add_argument("--comp", default="Luma,Chroma")
    ap.add_argument("--blocks", default=4096, type=int, help="blocks of the resident set")
    ap.add_argument("--iters", default=20, type=int)
    ap.add_argument("--warmup", default=3, type=int)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "train_step.txt"), help="the file the lines are written to")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("train_step_bench: no GPU - there is no CPU fallback")
    eng = engine.Engine(0)
    lines = ["a training step's ends and the whole step: the batch (pmp_batch_gather_device against host batches copied in), Adam (optim.Adam "
             "against torch.optim.Adam) and a train_QBD step, float32, hipEvents, %d calls after %d warm-up calls, %s" %
             (a.iters, a.warmup, torch.cuda.get_device_name(0)), ""]
    with torch.cuda.stream(torch.cuda.Stream()):        # a real stream: the library adopts it, and the events time what runs on it
        for comp in [c for c in a.comp.split(",") if c]:
            torch.cuda.synchronize()
            torch.cuda.empty_cache()
            got = bench(eng, comp, a.n, a.blocks, a.warmup, a.iters)
            print("\n".join(got), flush=True)
            lines += got
    eng.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
