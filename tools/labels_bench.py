"""Throughput of the GenMSBtMap label kernel (include/pmp.h: pmp_msbt_labels_device) on an MI355X; output kept in profiles/msbt_labels.txt.

    python tools/labels_bench.py [--blocks 65536] [--reps 5]

Valid synthetic partitions (synth.random_partition_maps, 8192 distinct blocks tiled to --blocks) per chroma factor, timed with device
pointers on torch's stream (median of --reps launches after a warm-up); then a 1024-block batch of worst-case blocks (labels that admit
every legal split: the leaf budget ends every region); and, on the CPU, the largest leaf count the restatement (tests/msbt_cases.py)
sees on 2000 of the valid blocks.
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402

import msbt_cases as K  # noqa: E402


def timed(eng, torch, cf, qt, bt, dire, reps):
    n = len(qt)
    d = [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (qt, bt, dire)]
    out = torch.empty((n, 3, 16, 16), dtype=torch.uint8, device="cuda"); st = torch.empty(n, dtype=torch.uint8, device="cuda")
    args = (cf, d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), n, out.data_ptr(), st.data_ptr())
    eng.set_stream(torch.cuda.current_stream().cuda_stream)
    eng.msbt_labels_device(*args)
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t = time.perf_counter()
        eng.msbt_labels_device(*args)
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t)
    eng.set_stream(None)
    return float(np.median(ts)), st.cpu().numpy()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=65536)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    import torch
    from pmp_vvc_tip2023_amd import engine
    eng = engine.Engine(0)
    print("device: %s" % torch.cuda.get_device_name(0))
    for cf in (1, 2):
        qt, bt, dire = K.valid_blocks(8192, 5000 + cf, cf)
        reps = (a.blocks + 8191) // 8192
        qt, bt, dire = (np.concatenate([x] * reps)[:a.blocks] for x in (qt, bt, dire))
        dt, st = timed(eng, torch, cf, qt, bt, dire, a.reps)
        print("valid cf %d: %d blocks in %.2f ms = %.0f blocks/s (status nonzero: %d)" % (cf, len(qt), dt * 1e3, len(qt) / dt,
                                                                                           int(np.count_nonzero(st))))
    for cf in (1, 2):
        qt, bt, dire = K.worst_blocks(1024)
        dt, st = timed(eng, torch, cf, qt, bt, dire, a.reps)
        print("worst case cf %d: 1024 blocks in %.1f ms (status bit 4 on %d blocks)" % (cf, dt * 1e3, int(np.count_nonzero(st & 4))))
    eng.close()
    for cf in (1, 2):
        qt, bt, dire = K.valid_blocks(2000, 5000 + cf, cf)
        stats = []
        K.restate_batch(qt, bt, dire, cf, stats=stats)
        print("largest leaf count per QT region, 2000 valid blocks cf %d: %d (%d regions, 99th percentile %d)"
              % (cf, max(stats), len(stats), int(np.percentile(stats, 99))))


if __name__ == "__main__":
    main()
