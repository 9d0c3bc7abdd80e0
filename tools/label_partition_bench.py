"""Throughput of the label-to-partition kernel (include/pmp.h: pmp_label_partition_device / _records_device) on an MI355X, next to the
label kernel (pmp_msbt_labels_device) on the same inputs in the same run; output kept in profiles/label_partition.txt.

    python tools/label_partition_bench.py [--blocks 65536] [--reps 9]

The inputs of tools/labels_bench.py: valid synthetic partitions (synth.random_partition_maps, 8192 distinct blocks tiled to --blocks) per
chroma factor, then a 1024-block batch of worst-case blocks (the leaf budget ends every region).  Device pointers on torch's stream;
after a warm-up of all three kernels the timed launches ALTERNATE between them (launch + synchronise, host clock), median of --reps.
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
    """-> ({kernel: median seconds}, status of the partition kernel, status of the label kernel)"""
    from pmp_vvc_tip2023_amd import _lib
    n = len(qt)
    d = [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (qt, bt, dire)]
    inp = (cf, d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), n)
    msbt = torch.empty((n, 3, 16, 16), dtype=torch.uint8, device="cuda")
    hor = torch.empty((n, 16, 16), dtype=torch.uint8, device="cuda"); ver = torch.empty_like(hor)
    rec = torch.empty((n, _lib.PMP_RECORD_BYTES), dtype=torch.uint8, device="cuda")
    st = [torch.empty(n, dtype=torch.uint8, device="cuda") for _ in range(3)]
    calls = {"labels": lambda: eng.msbt_labels_device(*inp, msbt.data_ptr(), st[0].data_ptr()),
             "partition": lambda: eng.label_partition_device(*inp, hor.data_ptr(), ver.data_ptr(), st[1].data_ptr()),
             "records": lambda: eng.label_partition_records_device(*inp, rec.data_ptr(), st[2].data_ptr())}
    eng.set_stream(torch.cuda.current_stream().cuda_stream)
    for f in calls.values():
        f()
    torch.cuda.synchronize()
    ts = {k: [] for k in calls}
    for _ in range(reps):
        for k, f in calls.items():
            t = time.perf_counter()
            f()
            torch.cuda.synchronize()
            ts[k].append(time.perf_counter() - t)
    eng.set_stream(None)
    assert torch.equal(rec[:, :256].reshape(n, 16, 16), hor) and torch.equal(st[1], st[2])
    return {k: float(np.median(v)) for k, v in ts.items()}, st[1].cpu().numpy(), st[0].cpu().numpy()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=65536)
    ap.add_argument("--reps", type=int, default=9)
    a = ap.parse_args()
    import torch
    from pmp_vvc_tip2023_amd import engine
    eng = engine.Engine(0)
    print("device: %s" % torch.cuda.get_device_name(0))
    for cf in (1, 2):
        qt, bt, dire = K.valid_blocks(8192, 5000 + cf, cf)
        reps = (a.blocks + 8191) // 8192
        qt, bt, dire = (np.concatenate([x] * reps)[:a.blocks] for x in (qt, bt, dire))
        dt, st, _ = timed(eng, torch, cf, qt, bt, dire, a.reps)
        n = len(qt)
        print("valid cf %d, %d blocks (status nonzero: %d):" % (cf, n, int(np.count_nonzero(st))))
        for k in ("labels", "partition", "records"):
            print("    %-9s %6.2f ms = %9.0f blocks/s  (%.2fx the label kernel's time)" % (k, dt[k] * 1e3, n / dt[k], dt[k] / dt["labels"]))
    for cf in (1, 2):
        qt, bt, dire = K.worst_blocks(1024)
        dt, st, st_l = timed(eng, torch, cf, qt, bt, dire, a.reps)
        print("worst case cf %d, 1024 blocks (status bit 4 on %d blocks; label kernel: %d):" % (cf, int(np.count_nonzero(st & 4)),
                                                                                                 int(np.count_nonzero(st_l & 4))))
        for k in ("labels", "partition", "records"):
            print("    %-9s %6.1f ms  (%.2fx the label kernel's time)" % (k, dt[k] * 1e3, dt[k] / dt["labels"]))
    eng.close()


if __name__ == "__main__":
    main()
