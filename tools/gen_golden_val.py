"""Generate tests/golden/g12_val.npz from the IMPORTED REFERENCE: the numbers of Metrics.validation_QBD / pre_validation / loss_func_*_val.

Run where the reference checkout is (CPU; tools/ref_harness.py shims .cuda()):   python tools/gen_golden_val.py
Inputs are rebuilt by tests/val_cases.py; only the reference's outputs are stored, per case of val_cases.CASES:
  <case>_vqbd  f64[15]        validation_QBD(loader, Net_Q, Net_BD, qp)
  <case>_pre0  f64[2]         pre_validation(loader, Net, 0, qp)
  <case>_pre1  f64[13]        pre_validation(loader, Net, 1, qp)
  <case>_loss_qbd, <case>_loss_msbd  f64[batches]   loss_func_QBD_val / loss_func_MSBD_val per batch
  ref_vs_f64                  the largest relative distance between a reference number above and the numpy restatement's
                              (val_cases: float32 terms, float64 sums): the reference's own float32 summation error
The loader is a list of batches cut in order (the reference's DataLoader shuffles), labels converted as Load_Pre_VP_Dataset converts
them (Metrics.py:127-135); the nets are stubs that return the case's logits for the block indices the batch carries as its input.
While generating, every hit-derived number (an accuracy: a ratio of integers) must equal the restatement's EXACTLY, and ref_vs_f64 must
stay below 1e-5: beyond that something other than float32 summation order is going on.
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, HERE)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import ref_harness  # noqa: E402
import val_cases as K  # noqa: E402


def loader(c, with_bd=True):
    """Batches as Load_Pre_VP_Dataset's tensors (Metrics.py:127-135); the 'input' is the batch's block indices."""
    ql = torch.FloatTensor(np.expand_dims(c["qt8"], 1) - 1)           # the loader's own expression: numpy subtracts on the u8 array
    bl = torch.FloatTensor(c["msbt"])
    dl = torch.FloatTensor(c["msdire"])
    out = []
    for o, m in K.batches(c):
        idx = torch.arange(o, o + m)
        out.append((idx, ql[o:o + m], bl[o:o + m], dl[o:o + m]) if with_bd else (idx, ql[o:o + m]))
    return out, ql


def main():
    _, Metrics, _, _ = ref_harness.load()
    out = {}
    worst = 0.0
    for name in K.CASES:
        c = K.make(name)
        qp = c["qp"]
        qt = torch.from_numpy(c["qt"]).reshape(-1, 1, 8, 8)
        bt, dire = torch.from_numpy(c["bt"]), torch.from_numpy(c["dire"])
        net_q = lambda idx: qt[idx]
        net_bd = lambda idx, q: tuple(torch.stack([bt[idx, k], dire[idx, k]], dim=1) for k in range(3))
        ld, ql = loader(c)
        if (c["qt8"] == 0).any():
            assert float(ql.max()) == 255.0, "the loader no longer wraps raw qtDepth 0 to 255.0"
        vqbd = np.array(Metrics.validation_QBD(ld, net_q, net_bd, qp), np.float64)
        pre0 = np.array(Metrics.pre_validation(loader(c, False)[0], net_q, 0, qp), np.float64)
        pre1 = np.array(Metrics.pre_validation(ld, net_bd, 1, qp), np.float64)
        lq, lm = [], []
        for idx, a, b, d in ld:
            o0, o1, o2 = net_bd(idx, None)
            lq.append(float(Metrics.loss_func_QBD_val(net_q(idx), o0, o1, o2, a, b, d, qp)))
            lm.append(float(Metrics.loss_func_MSBD_val(o0, o1, o2, b, d, qp)))
        out[name + "_vqbd"], out[name + "_pre0"], out[name + "_pre1"] = vqbd, pre0, pre1
        out[name + "_loss_qbd"], out[name + "_loss_msbd"] = np.array(lq), np.array(lm)
        # against the restatement
        dist = 0.0
        for mode, ref, losses in (("qbd", vqbd, lq), ("q", pre0, None), ("bd", pre1, lm)):
            S, ns = K.case_stats(c, mode)
            mine, loss = K.numbers(S, ns, mode)
            ex = K.EXACT[mode]
            assert np.array_equal(mine[ex], ref[ex]), (name, mode, mine[ex], ref[ex])
            dist = max(dist, K.rel_dist(ref, mine))
            if losses is not None:
                dist = max(dist, K.rel_dist(losses, loss))
        print("%-12s qp %d, %d blocks in batches of %d: ref vs float64 restatement %.3g" % (name, qp, c["n"], c["batch"], dist), flush=True)
        worst = max(worst, dist)
    assert worst < 1e-5, worst
    out["ref_vs_f64"] = np.float64(worst)
    print("ref_vs_f64 = %.6g" % worst)
    np.savez_compressed(K.GOLDEN, **out)
    print("wrote", K.GOLDEN, os.path.getsize(K.GOLDEN), "bytes")


if __name__ == "__main__":
    main()
