"""Cost of validation on an MI355X (include/pmp.h: pmp_val_stats_device, Engine.validation_QBD); output kept in profiles/val_stats.txt.

    python tools/val_bench.py [--blocks 4096] [--reps 7] [--qp 22] [--only-stats]
    python tools/val_bench.py --confusion | --pre0        (output kept in profiles/val_confusion.txt)

(i) one pmp_val_stats_device call on --blocks luma blocks of logits: hipEvent time around the call on the context's stream (block
kernel + reduction), median of single calls after a warm-up, and 200 calls back to back between two events (a single call is a window
of microseconds: the loop is the figure to quote); --only-stats stops here (for a `rocprofv3 --kernel-trace --stats` run of its own,
which gives the two kernels' own durations); (ii) in the same run, the bare pmp_infer_device step on the same blocks (wall
clock around call + pmp_synchronize, median), then Engine.validation_QBD on them at batch 200 and at batch --blocks, wall clock, median,
as blocks/s.  Engine.validation_QBD's time includes what the bare step leaves out: uploading blocks and labels, allocating the logits,
and reading the statistics back; the tool prints that part on its own (the same call with logits given, i.e. without the nets).

--confusion: pmp_val_confusion_device next to pmp_val_stats_device on the same logits and labels in one process, at 200 and at 4096
blocks, each as 200 calls back to back between two hipEvents on the context's stream; both read the same bytes per block.
--pre0: Engine.pre_validation(pred_id=0) on --blocks luma blocks at batch 200, wall clock, median - the QT net's validation, which
runs on pmp_infer_q_device here and ran a whole inference step (the MTT net is 75 % of the FLOPs) before that call existed.  The leg
uses nothing newer than pre_validation itself, so the same file, copied into an older checkout's tools/, times that checkout too.
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402

import val_cases as K  # noqa: E402


def med(f, reps):
    f()
    ts = []
    for _ in range(reps):
        t = time.perf_counter()
        f()
        ts.append(time.perf_counter() - t)
    return float(np.median(ts))


def loop_us(st, call, calls=200):
    """hipEvents around `calls` calls back to back on the torch stream `st` -> microseconds per call"""
    import torch
    call()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(st)
    for _ in range(calls):
        call()
    e1.record(st)
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / calls


def confusion_leg(a):
    import torch
    import confusion_cases as X
    from pmp_vvc_tip2023_amd import engine
    eng = engine.Engine(0)
    print("device: %s" % torch.cuda.get_device_name(0))
    st = torch.cuda.Stream()
    eng.set_stream(st.cuda_stream)
    for n in (200, 4096):
        c = X.in_range(n, 21)
        d = [torch.from_numpy(c[k]).cuda() for k in X.ORDER]
        six = [t.data_ptr() for t in d]
        S = torch.zeros(20, dtype=torch.float64, device="cuda")
        C = torch.zeros(X.NCOUNTS, dtype=torch.int64, device="cuda")
        B = torch.zeros((n, X.NCOUNTS), dtype=torch.int16, device="cuda")
        torch.cuda.synchronize()
        for r in range(3):
            t_s = loop_us(st, lambda: eng.val_stats_device(a.qp, *six, n, S.data_ptr()))
            t_c = loop_us(st, lambda: eng.val_confusion_device(*six, n, C.data_ptr()))
            t_b = loop_us(st, lambda: eng.val_confusion_device(*six, n, C.data_ptr(), B.data_ptr()))
            print("%4d blocks (%.2f MB read), run %d: pmp_val_stats_device %.1f us, pmp_val_confusion_device %.1f us (%.2f x), with "
                  "d_block_counts %.1f us" % (n, n * (64 * 4 + 2 * 768 * 4 + 64 + 2 * 768) / 1e6, r, t_s, t_c, t_c / t_s, t_b))
        eng.synchronize()
        assert np.array_equal(C.cpu().numpy().reshape(7, 5, 5), X.counts(**c))
    eng.set_stream(None)
    eng.close()


def pre0_leg(a):
    import torch
    from pmp_vvc_tip2023_amd import engine, synth
    n = a.blocks
    eng = engine.Engine(0, allow_synthetic_mtt=True)
    y, _, _ = synth.recipe_r_blocks(n, 11)
    qt8, _, _ = K.labels(n, 12)
    t = med(lambda: eng.pre_validation("Luma", a.qp, 0, y, qt8, batch_size=200), a.reps)
    res = eng.pre_validation("Luma", a.qp, 0, y, qt8, batch_size=200)
    print("device: %s; Engine.pre_validation(pred_id=0), %d luma blocks, QP %d, batch 200, %s: %.2f ms = %.0f blocks/s; MTT net loaded: %s; "
          "[L1, accuracy] = %r" % (torch.cuda.get_device_name(0), n, a.qp, eng.get_precision(), t * 1e3, n / t,
                                   eng.has_weights("Luma_MSBD", a.qp), res))
    eng.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--qp", type=int, default=22)
    ap.add_argument("--only-stats", action="store_true")
    ap.add_argument("--confusion", action="store_true")
    ap.add_argument("--pre0", action="store_true")
    a = ap.parse_args()
    if a.confusion or a.pre0:
        if a.confusion:
            confusion_leg(a)
        if a.pre0:
            pre0_leg(a)
        return
    import torch
    from pmp_vvc_tip2023_amd import engine, synth
    n, qp = a.blocks, a.qp
    eng = engine.Engine(0, allow_synthetic_mtt=True)
    print("device: %s; %d luma blocks, QP %d, datapath %s" % (torch.cuda.get_device_name(0), n, qp, eng.get_precision()))
    y, _, _ = synth.recipe_r_blocks(n, 11)
    qt8, msbt, msdire = K.labels(n, 12)
    eng.load("Luma", qp)
    d_y = torch.from_numpy(y).cuda()
    lab = [torch.from_numpy(x).cuda() for x in (qt8, msbt, msdire)]
    qt = torch.empty((n, 64), device="cuda"); bt = torch.empty((n, 768), device="cuda"); dire = torch.empty((n, 768), device="cuda")
    S = torch.zeros(20, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()

    def infer():
        eng.infer_device("Luma", qp, d_y.data_ptr(), None, None, n, qt.data_ptr(), bt.data_ptr(), dire.data_ptr())
        eng.synchronize()
    t_inf = med(infer, a.reps)
    print("bare pmp_infer_device step: %.2f ms = %.0f blocks/s" % (t_inf * 1e3, n / t_inf))

    # (i) the statistics call alone, hipEvents on the context's stream: a torch stream of our own handed to the context (torch's
    # default stream is the null handle, which pmp_set_stream takes as "the context's own stream": events on it would time nothing)
    st = torch.cuda.Stream()
    eng.set_stream(st.cuda_stream)
    args = (qp, qt.data_ptr(), bt.data_ptr(), dire.data_ptr(), lab[0].data_ptr(), lab[1].data_ptr(), lab[2].data_ptr(), n, S.data_ptr())
    eng.val_stats_device(*args)
    torch.cuda.synchronize()
    us = []
    for _ in range(max(a.reps, 21)):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(st)
        eng.val_stats_device(*args)
        e1.record(st)
        e1.synchronize()
        us.append(e0.elapsed_time(e1) * 1e3)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(st)
    for _ in range(200):
        eng.val_stats_device(*args)
    e1.record(st)
    e1.synchronize()
    loop_us = e0.elapsed_time(e1) * 1e3 / 200
    eng.set_stream(None)
    print("pmp_val_stats_device, %d blocks: %.1f us per call over 200 calls back to back (hipEvents around the loop)" % (n, loop_us))
    print("pmp_val_stats_device, %d blocks (%.1f MB read): median %.1f us, min %.1f us (hipEvents, %d calls)"
          % (n, n * (64 * 4 + 2 * 768 * 4 + 64 + 2 * 768) / 1e6, float(np.median(us)), min(us), len(us)))
    t_host = med(lambda: (eng.val_stats_device(*args), eng.synchronize()), a.reps)
    print("the same call, wall clock with pmp_synchronize: %.1f us" % (t_host * 1e6))

    if a.only_stats:
        eng.close()
        return

    # (ii) validation end to end
    lg = (qt.cpu().numpy(), bt.cpu().numpy(), dire.cpu().numpy())
    for batch in (200, n):
        t = med(lambda: eng.validation_QBD("Luma", qp, y, qt8, msbt, msdire, batch_size=batch), a.reps)
        t0 = med(lambda: eng.validation_QBD("Luma", qp, None, qt8, msbt, msdire, batch_size=batch, logits=lg), a.reps)
        nb = (n + batch - 1) // batch
        print("Engine.validation_QBD batch %d (%d batches): %.2f ms = %.0f blocks/s; %.2f x the bare step (+%.2f ms); "
              "without the nets (logits given: uploads, statistics, read-back) %.2f ms"
              % (batch, nb, t * 1e3, n / t, t / t_inf, (t - t_inf) * 1e3, t0 * 1e3))
    # the nets at batch 200 on their own: the bare step cut the same way
    def infer200():
        for o in range(0, n, 200):
            m = min(200, n - o)
            eng.infer_device("Luma", qp, d_y.data_ptr() + o * 68 * 68, None, None, m, qt.data_ptr() + o * 256, bt.data_ptr() + o * 3072,
                             dire.data_ptr() + o * 3072)
        eng.synchronize()
    t200 = med(infer200, a.reps)
    print("pmp_infer_device in calls of 200 blocks, one synchronize: %.2f ms = %.0f blocks/s" % (t200 * 1e3, n / t200))
    print("saturation re-runs: %d" % eng.saturation_reruns())
    eng.close()


if __name__ == "__main__":
    main()
