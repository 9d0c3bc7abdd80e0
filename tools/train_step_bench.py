"""Time the ends of a training step and the whole step, and write profiles/train_step.txt:
  (a) the batch: pmp_batch_gather_device from a set resident on the GPU as bytes (dataset.DeviceDataset), next to what
      Load_Pre_VP_Dataset's DataLoader does per step - rows of the host-side float32 tensors gathered into pinned memory and copied in;
  (b) the optimiser: optim.Adam.step (one launch) next to torch.optim.Adam.step on the same parameters and gradients, in the order
      torch / this library / torch;
  (c) a whole train_QBD step: train_qbd.Trainer.step on a batch gathered on the device, next to the composition without this work -
      tools/qtail_grad_bench.py's joint step (the nets and the loss through this library, the batch already on the device) and
      torch.optim.Adam.step.
No eager reference net runs here; torch's optimiser is not one.
  --ddp instead times what data-parallel training (grad_sync.py, train_qbd --gpus N) adds to a step, in ONE process on one GPU, and
  writes profiles/train_step_ddp.txt: pmp_grad_pack_device, the RCCL all_gather_into_tensor of a ONE-rank group (its launch and a
  device copy: no link is crossed), pmp_grad_sum_device over 2 and over 8 buckets, GradSync.sync as a whole, and Trainer.step with
  and without it.  These are the costs a rank pays on top of its step; what a gather across GPUs costs, and so the speed-up, is NOT
  measured here - that needs a node with several GPUs.

  --guard instead times what the divergence guard (--clipNorm 1 --skipNonFinite: optim.Adam's max_grad_norm and skip_nonfinite) adds
  to a train_QBD step, in one process, and writes profiles/train_step_guard.txt: the unguarded step, the guarded step and the
  unguarded step again, and the guard call, the guarded and the plain Adam call alone.  --root DIR imports the package from another
  tree of this project - the parent commit's, built, to time ITS step the same way; a tree without the guard gets the unguarded
  legs alone.  --append adds to the file, so that parent, this commit, parent stand in one file.

    python tools/train_step_bench.py [--n 200] [--comp Luma,Chroma] [--blocks 4096] [--iters 20] [--warmup 3] [--out FILE] [--ddp]
           [--guard [--root DIR] [--append]]

Times are hipEvent times around `iters` back-to-back calls (20 * iters for the batch and for Adam, which take microseconds) after
`warmup` calls, a torch.cuda.synchronize() between every two legs;
for the host batches that interval holds the host's gathering too, as a training loop waits for it.  No ratio is judged; a line where
this library is slower is marked SLOWER.
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PACKAGE_ROOT = ROOT                         # --root DIR: the tree the package is imported from
if "--root" in sys.argv[1:-1]:
    PACKAGE_ROOT = os.path.abspath(sys.argv[sys.argv.index("--root") + 1])
sys.path.insert(0, PACKAGE_ROOT)

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


def synthetic_set(luma, blocks):
    """-> (what validation.read_set would return for a set of `blocks` random blocks, y, u, v)"""
    rng = np.random.default_rng(6100 + luma)
    y = rng.integers(0, 256, (blocks, 68, 68), dtype=np.uint8)
    u, v = (rng.integers(0, 256, (blocks, 34, 34), dtype=np.uint8) for _ in range(2))
    files = {"blocks": y if luma else (y, u, v), "qt8": rng.integers(1, 5, (blocks, 8, 8), dtype=np.uint8),
             "msbt": rng.integers(0, 4, (blocks, 3, 16, 16), dtype=np.uint8), "msdire": rng.integers(-1, 2, (blocks, 3, 16, 16)).astype(np.int8),
             "n": blocks}
    return files, y, u, v


def bench_ddp(eng, comp, n, blocks, warmup, iters):
    """What grad_sync adds to a step, on a forced one-rank RCCL group"""
    import torch.distributed as dist
    from pmp_vvc_tip2023_amd import grad_sync, parallel
    from pmp_vvc_tip2023_amd.torch_call import P, run
    luma = comp == "Luma"
    dev = torch.device("cuda", 0)
    os.environ.pop("PMP_DIST_BACKEND", None)
    parallel.init_process_group(dev, force=True)
    assert dist.get_backend() == "nccl" and dist.get_world_size() == 1
    files = synthetic_set(luma, blocks)[0]
    train = dataset.DeviceDataset(eng, None, comp, 22, "Train", 2, 0, files=files)
    d_order = dataset.permutation(blocks, True, 1, 0).cuda()
    nb = blocks // n
    at = [0]

    def batch():
        b = at[0] = (at[0] + 1) % nb
        return train.gather(d_order[b * n:(b + 1) * n], n)

    args = train_qbd.build_parser().parse_args(["--predID", "2", "--lr", "1e-4", "--batchSize", str(n)] + (["--isLuma"] if luma else []))
    torch.manual_seed(6200 + luma)
    trainer = train_qbd.Trainer(eng, args, comp, {}, 0)
    t_plain = timed(lambda: trainer.step(batch()), warmup, iters); torch.cuda.synchronize()
    trainer.data_parallel()
    sync = trainer.sync
    t_sync_step = timed(lambda: trainer.step(batch(), n), warmup, iters); torch.cuda.synchronize()
    trainer.sync = None
    t_plain2 = timed(lambda: trainer.step(batch()), warmup, iters); torch.cuda.synchronize()
    trainer.sync = sync
    values = trainer.step(batch(), n)                      # leaves every .grad a view of the receive area
    small = 20 * iters
    grads = [p.grad for p in sync.params]
    t_pack = timed(lambda: run(eng, dev, lambda: eng.grad_pack_device([P(g) for g in grads], sync.counts, P(sync.bucket))), warmup, small); torch.cuda.synchronize()
    t_gather = timed(lambda: dist.all_gather_into_tensor(sync.recv, sync.bucket), warmup, small); torch.cuda.synchronize()
    t_sum = {}
    for w in (2, 8):
        area = torch.zeros((w, sync.total), dtype=torch.float32, device=dev)
        src = [P(area[r]) for r in range(w)]
        t_sum[w] = timed(lambda: run(eng, dev, lambda: eng.grad_sum_device(src, sync.total, src[0])), warmup, small); torch.cuda.synchronize()
    t_whole = timed(lambda: sync.sync([0], values), warmup, small); torch.cuda.synchronize()
    train.check()
    dist.destroy_process_group()
    mb = sync.total * 4 / 1e6
    head = "%s, n %d, %d tensors, a bucket of %d floats (%.2f MB)" % (comp, n, len(sync.params), sync.total, mb)
    return [head,
            "  pmp_grad_pack_device                                   %9.3f ms" % t_pack,
            "  all_gather_into_tensor, RCCL, ONE rank (no link crossed) %7.3f ms" % t_gather,
            "  pmp_grad_sum_device over 2 buckets, in place           %9.3f ms" % t_sum[2],
            "  pmp_grad_sum_device over 8 buckets, in place           %9.3f ms   (%.0f GB/s of %.1f MB read and written)" %
            (t_sum[8], 9 * mb / t_sum[8], 9 * mb),
            "  GradSync.sync, one rank: pack, gather, the numbers' gather %5.3f ms" % t_whole,
            "  train_QBD step without a process group                 %9.3f ms, again %9.3f ms" % (t_plain, t_plain2),
            "  train_QBD step with GradSync on a one-rank RCCL group  %9.3f ms   (+%.3f ms, %.2f %%)" %
            (t_sync_step, t_sync_step - min(t_plain, t_plain2), 100 * (t_sync_step / min(t_plain, t_plain2) - 1))]


def bench_guard(eng, comp, n, blocks, warmup, iters):
    """The train_QBD step without the guard, with it, and without it again; then the guard's calls alone on the step's gradients"""
    from pmp_vvc_tip2023_amd.torch_call import P, run
    luma = comp == "Luma"
    dev = torch.device("cuda", 0)
    files = synthetic_set(luma, blocks)[0]
    train = dataset.DeviceDataset(eng, None, comp, 22, "Train", 2, 0, files=files)
    d_order = dataset.permutation(blocks, True, 1, 0).cuda()
    nb = blocks // n
    at = [0]

    def batch():
        b = at[0] = (at[0] + 1) % nb
        return train.gather(d_order[b * n:(b + 1) * n], n)

    flags = ["--predID", "2", "--lr", "1e-4", "--batchSize", str(n)] + (["--isLuma"] if luma else [])
    has_guard = hasattr(train_qbd, "guard_kwargs")
    torch.manual_seed(6200 + luma)
    plain = train_qbd.Trainer(eng, train_qbd.build_parser().parse_args(flags), comp, {}, 0)
    t_a1 = timed(lambda: plain.step(batch()), warmup, iters); torch.cuda.synchronize()
    head = "%s train_QBD step, n %d: gather + nets + loss + Adam" % (comp, n)
    if not has_guard:
        t_a2 = timed(lambda: plain.step(batch()), warmup, iters); torch.cuda.synchronize()
        train.check()
        return ["%-52s ms: unguarded %9.3f | unguarded again %9.3f    (runs apart by %.1f %%)   [this tree has no guard]" %
                (head, t_a1, t_a2, 100 * abs(t_a1 - t_a2) / min(t_a1, t_a2))]
    torch.manual_seed(6200 + luma)
    guarded = train_qbd.Trainer(eng, train_qbd.build_parser().parse_args(flags + ["--clipNorm", "1", "--skipNonFinite"]), comp, {}, 0)
    guarded.begin_epoch()
    t_g = timed(lambda: guarded.step(batch()), warmup, iters); torch.cuda.synchronize()
    t_a2 = timed(lambda: plain.step(batch()), warmup, iters); torch.cuda.synchronize()
    state = guarded.optimizer.guard_state()
    t_o = min(t_a1, t_a2)
    lines = ["%-52s ms: unguarded %9.3f | --clipNorm 1 --skipNonFinite %9.3f | unguarded %9.3f    the guard adds %+.3f ms (%+.2f %%) "
             "(the unguarded runs apart by %.1f %%)" % (head, t_a1, t_g, t_a2, t_g - t_o, 100 * (t_g / t_o - 1), 100 * abs(t_a1 - t_a2) / t_o),
             "  the guarded steps: %d, skipped %d, clipped %d, largest gradient norm %.6g" % (state["steps"], state["skipped"], state["clipped"], state["max_norm"])]
    # the calls alone, on the last step's gradients and on copies of the parameters and moments
    ps = [p for net in guarded.nets.values() for p in net.parameters() if p.grad is not None]
    gs = [p.grad for p in ps]
    counts = [p.numel() for p in ps]
    cp, ms, vs = ([torch.zeros_like(p) for p in ps] for _ in range(3))
    scratch = torch.empty(eng.grad_guard_scratch_bytes(counts) // 8, dtype=torch.float64, device=dev)
    record, counters = torch.zeros(4, dtype=torch.float64, device=dev), torch.zeros(6, dtype=torch.int64, device=dev)
    small = 20 * iters
    t_guard = timed(lambda: run(eng, dev, lambda: eng.grad_guard_device([P(g) for g in gs], counts, P(scratch), P(record), P(counters), max_norm=1.0,
                                                                        skip_nonfinite=True)), warmup, small); torch.cuda.synchronize()
    tensors = ([P(t) for t in cp], [P(g) for g in gs], [P(t) for t in ms], [P(t) for t in vs], counts, 7)
    t_adam = timed(lambda: run(eng, dev, lambda: eng.adam_step_device(*tensors)), warmup, small); torch.cuda.synchronize()
    t_gadam = timed(lambda: run(eng, dev, lambda: eng.adam_step_guarded_device(*tensors, P(record))), warmup, small); torch.cuda.synchronize()
    train.check()
    lines += ["  pmp_grad_guard_device, %d tensors, %d elements, %d tiles: %9.3f ms   (two launches)" %
              (len(ps), sum(counts), eng.grad_guard_scratch_bytes(counts) // 16, t_guard),
              "  pmp_adam_step_device %9.3f ms | pmp_adam_step_guarded_device %9.3f ms   (through torch_call.run, the host's time included)" % (t_adam, t_gadam)]
    return lines


def bench(eng, comp, n, blocks, warmup, iters):
    luma = comp == "Luma"
    files, y, u, v = synthetic_set(luma, blocks)
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
    ap.add_argument("--out", default=None, help="the file the lines are written to (profiles/train_step.txt; with --ddp profiles/train_step_ddp.txt)")
    ap.add_argument("--ddp", action="store_true", help="time what data-parallel training adds to a step instead (one process, a one-rank RCCL group)")
    ap.add_argument("--guard", action="store_true", help="time what the divergence guard adds to a step instead")
    ap.add_argument("--root", default=None, help="with --guard: import the package from this tree (the parent commit's, built)")
    ap.add_argument("--append", action="store_true", help="add to --out instead of replacing it")
    a = ap.parse_args()
    a.out = a.out or os.path.join(ROOT, "profiles", "train_step_ddp.txt" if a.ddp else "train_step_guard.txt" if a.guard else "train_step.txt")
    if not torch.cuda.is_available():
        raise SystemExit("train_step_bench: no GPU - there is no CPU fallback")
    eng = engine.Engine(0)
    ddp_head = ("what data-parallel training adds to a training step, in ONE process on one GPU (a forced one-rank RCCL group): the gather crosses no "
                "link, so these are a rank's own costs, NOT a speed-up and not the cost of a gather across GPUs, which no run here has "
                "measured; float32, hipEvents, %d calls (step) or %d calls (the rest) after %d warm-up calls, %s" %
                (a.iters, 20 * a.iters, a.warmup, torch.cuda.get_device_name(0)))
    lines = [ddp_head, ""] if a.ddp else ["a training step's ends and the whole step: the batch (pmp_batch_gather_device against host batches copied in), Adam (optim.Adam "
             "against torch.optim.Adam) and a train_QBD step, float32, hipEvents, %d calls after %d warm-up calls, %s" %
             (a.iters, a.warmup, torch.cuda.get_device_name(0)), ""]
    if a.guard:
        lines = ["what the divergence guard adds to a train_QBD step, one process; the package of %s; float32, hipEvents, %d calls (step) or %d calls "
                 "(the calls alone) after %d warm-up calls, %s" % ("this tree" if PACKAGE_ROOT == ROOT else "the tree given with --root", a.iters,
                                                                    20 * a.iters, a.warmup, torch.cuda.get_device_name(0)), ""]
    if a.ddp and a.comp == "Luma,Chroma":
        a.comp = "Luma"                                  # one process group to a process: one component to a run
    with torch.cuda.stream(torch.cuda.Stream()):        # a real stream: the library adopts it, and the events time what runs on it
        for comp in [c for c in a.comp.split(",") if c]:
            torch.cuda.synchronize()
            torch.cuda.empty_cache()
            got = (bench_ddp if a.ddp else bench_guard if a.guard else bench)(eng, comp, a.n, a.blocks, a.warmup, a.iters)
            print("\n".join(got), flush=True)
            lines += got
    eng.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a" if a.append else "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
