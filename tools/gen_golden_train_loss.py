"""Generate tests/golden/g14_train_loss.npz from the IMPORTED REFERENCE: Train_QBD's losses and torch's gradients of them.

Run where the reference checkout is (CPU; tools/ref_harness.py sets up the path):   python tools/gen_golden_train_loss.py
Inputs are rebuilt by tests/train_loss_cases.py; only the reference's outputs are stored, per case of train_loss_cases.CASES and form:
  <case>_qbd_loss, _g_qt, _g_bt, _g_dire   Train_QBD.loss_func_QBD(...) and .backward()
  <case>_bd_loss, _g_bt, _g_dire           Train_QBD.loss_func_MSBD(...)
  <case>_q_loss, _g_qt                     Train_QBD.L1_Loss(qt_out, qt_label)        (pre_train_Q)
  ref_vs_f64_loss     the largest relative distance between a reference loss and the numpy restatement's (train_loss_cases: float32
                      terms, float64 sums): the reference's own float32 summation error
  ref_vs_f64_grad     the largest |ref - mine| / max |ref| over the gradient tensors: the reference's float32 products against the
                      restatement's float64 arithmetic rounded once
The reference's argparse sits under `if __name__ == '__main__'` and its loss functions read the module global `args`, which is set here
per case.  Labels are converted as Load_Pre_VP_Dataset converts them (Metrics.py:127-135); the heads are built from leaf tensors in the
library's layouts, so the gradients come back in those layouts.
While generating, wherever the reference's gradient is exactly 0 or NaN the restatement's must be too (and the other way round), and
both distances must stay below 1e-5: beyond that something other than rounding differs.
"""
import argparse
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, HERE)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import ref_harness  # noqa: E402
import train_loss_cases as K  # noqa: E402
import val_cases as V  # noqa: E402


def reference(T, c, mode):
    """-> (loss float64, {"qt" / "bt" / "dire": float32 gradients}) of the reference on the whole case as one batch."""
    T.args = argparse.Namespace(qp=c["qp"], **K.lam_of(c, mode))
    ql = torch.FloatTensor(np.expand_dims(c["qt8"], 1) - 1)           # the loader's own expression: numpy subtracts on the u8 array
    bl, dl = torch.FloatTensor(c["msbt"]), torch.FloatTensor(c["msdire"])
    qt = torch.from_numpy(c["qt"].copy()).reshape(-1, 1, 8, 8).requires_grad_()
    bt = torch.from_numpy(c["bt"].copy()).requires_grad_()
    dire = torch.from_numpy(c["dire"].copy()).requires_grad_()
    heads = [torch.stack([bt[:, k], dire[:, k]], dim=1) for k in range(3)]
    is_luma = c["comp"] == "Luma"
    if mode == "qbd":
        loss = T.loss_func_QBD(qt, heads[0], heads[1], heads[2], ql, bl, dl, is_luma)
    elif mode == "bd":
        loss = T.loss_func_MSBD(heads[0], heads[1], heads[2], bl, dl, is_luma)
    else:
        loss = T.L1_Loss(qt, ql)
    loss.backward()
    g = {}
    if mode in ("qbd", "q"):
        g["qt"] = qt.grad.reshape(-1, 8, 8).numpy().copy()
    if mode in ("qbd", "bd"):
        g["bt"], g["dire"] = bt.grad.numpy().copy(), dire.grad.numpy().copy()
    return float(loss.item()), g


def main():
    ref_harness.load()
    import Train_QBD as T
    out = {}
    worst_loss = worst_grad = 0.0
    blocks = 0
    for name in K.CASES:
        c = K.make(name)
        blocks += c["n"]
        if (c["qt8"] == 0).any():
            assert float((np.expand_dims(c["qt8"], 1) - 1).max()) == 255.0, "the loader no longer wraps raw qtDepth 0 to 255.0"
        for mode in K.MODES:
            loss, g = reference(T, c, mode)
            kw, lam = K.kw_of(c, mode), K.lam_of(c, mode)
            mine_loss = K.loss_value(K.terms(c["comp"], c["qp"], **kw), lam, c["n"])
            mine = K.grads(c["comp"], c["qp"], lam, c["n"], **kw)
            out["%s_%s_loss" % (name, mode)] = np.float64(loss)
            dl = V.rel_dist([loss], [mine_loss])
            dg = 0.0
            for key, ref in g.items():
                out["%s_%s_g_%s" % (name, mode, key)] = ref
                assert K.same_zero_nan_pattern(ref, mine[key]), (name, mode, key, "zero / NaN pattern of the gradient differs")
                dg = max(dg, K.grad_dist(ref, mine[key]))
            print("%-16s %-3s n %2d: loss %-12.8g ref vs float64 restatement: loss %.3g, gradients %.3g" % (name, mode, c["n"], loss, dl, dg), flush=True)
            worst_loss, worst_grad = max(worst_loss, dl), max(worst_grad, dg)
    assert blocks <= 64, blocks
    assert worst_loss < 1e-5 and worst_grad < 1e-5, (worst_loss, worst_grad)
    out["ref_vs_f64_loss"], out["ref_vs_f64_grad"] = np.float64(worst_loss), np.float64(worst_grad)
    print("ref_vs_f64_loss = %.6g   ref_vs_f64_grad = %.6g   (%d blocks)" % (worst_loss, worst_grad, blocks))
    np.savez_compressed(K.GOLDEN, **out)
    print("wrote", K.GOLDEN, os.path.getsize(K.GOLDEN), "bytes")


if __name__ == "__main__":
    main()
