"""Time pmp_train_loss_device (loss + logit gradients, one launch) next to torch's eager evaluation of the same loss and its backward.

    python tools/train_loss_bench.py --n 200 --comp Luma --qp 22 [--lamb "lambb0=0.8,lambresb2=0"] [--iters 200] [--warmup 20] [--out FILE]

Both sides start from the same device tensors in the library's layouts (qt f32[n,8,8], bt / dire f32[n,3,16,16]; labels uint8 / int8 for
the kernel, the loader's float tensors for torch) and end with the loss and the three gradient tensors on the device.  The torch side is
the plain module below, written from include/pmp.h; its loss and gradients are compared with the kernel's before anything is timed.
Times are hipEvent times around `iters` back-to-back calls after `warmup` calls, per call.  --n and --comp take comma-separated lists.
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from pmp_vvc_tip2023_amd import engine  # noqa: E402

LUMA_MAT = 0.5 * np.array([[1.0, 0.73, 0.15], [2.43, 0.35, 0.10], [0.96, 0.23, 0.07], [0.59, 0.16, 0.05]])
CHROMA_MAT = 0.5 * np.array([[17.83, 0.49, 0.11], [1.20, 0.25, 0.07], [0.58, 0.17, 0.05], [0.38, 0.12, 0.04]])


class EagerLoss(torch.nn.Module):
    """loss_func_QBD of include/pmp.h in eager torch: L1 means, weights w_k = dl_k^2 + M[row][k] (w_0 = 1 at qp 22), ten lambdas."""

    def __init__(self, comp, qp, lam):
        super().__init__()
        self.row = (LUMA_MAT if comp == "Luma" else CHROMA_MAT)[int((qp - 22) / 5)]
        self.qp, self.lam = qp, lam
        self.l1 = torch.nn.L1Loss()

    def forward(self, qt, bt, dire, ql, bl, dl):
        L, l1 = self.lam, self.l1
        w = [dl[:, k] * dl[:, k] + float(self.row[k]) for k in range(3)]
        if self.qp == 22:
            w[0] = 1.0
        loss = L.lambq * l1(qt, ql)
        for k in range(3):
            loss = loss + L.lambb[k] * l1(bt[:, k], bl[:, k]) + L.lambd[k] * l1(w[k] * dire[:, k], w[k] * dl[:, k])
            if k == 0:
                loss = loss + L.lambresb[0] * l1(w[0] * bt[:, 0], w[0] * bl[:, 0])
            else:
                loss = loss + L.lambresb[k] * l1(w[k] * (bt[:, k] - bt[:, k - 1]), w[k] * (bl[:, k] - bl[:, k - 1]))
        return loss


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
    return a.elapsed_time(b) / iters * 1e3          # microseconds per call


def one(eng, comp, qp, n, lam, warmup, iters):
    rng = np.random.default_rng(n)
    qt8 = torch.from_numpy(rng.integers(1, 5, (n, 8, 8)).astype(np.uint8)).cuda()
    msbt = torch.from_numpy(np.cumsum(rng.integers(0, 2, (n, 3, 16, 16)), axis=1).astype(np.uint8)).cuda()
    msdire = torch.from_numpy(rng.integers(-1, 2, (n, 3, 16, 16)).astype(np.int8)).cuda()
    ql, bl, dl = (qt8 - 1).float(), msbt.float(), msdire.float()
    qt = (ql + 0.45 * torch.randn_like(ql)).requires_grad_()
    bt = (bl + 0.45 * torch.randn_like(bl)).requires_grad_()
    dire = (dl + 0.45 * torch.randn_like(dl)).requires_grad_()
    out = torch.empty(14, dtype=torch.float64, device="cuda")
    g = [torch.empty_like(t) for t in (qt, bt, dire)]
    eng.set_stream(torch.cuda.current_stream().cuda_stream)

    def ours():
        eng.train_loss_device(comp, qp, qt.data_ptr(), bt.data_ptr(), dire.data_ptr(), qt8.data_ptr(), msbt.data_ptr(), msdire.data_ptr(), n,
                              out.data_ptr(), out.data_ptr() + 104, g[0].data_ptr(), g[1].data_ptr(), g[2].data_ptr(), params=lam)

    mod = EagerLoss(comp, qp, lam)

    def eager():
        for t in (qt, bt, dire):
            t.grad = None
        loss = mod(qt, bt, dire, ql, bl, dl)
        loss.backward()
        return loss

    ours()
    loss = eager()
    torch.cuda.synchronize()
    loss = float(loss.detach())
    dl_ = abs(float(out[13]) - loss) / abs(loss)
    dg = max(float((a - t.grad).abs().max() / t.grad.abs().max()) for a, t in zip(g, (qt, bt, dire)))
    if dl_ > 1e-5 or dg > 1e-5:
        raise SystemExit("kernel and eager torch disagree: loss %.3g, gradients %.3g" % (dl_, dg))
    t_ours, t_eager = timed(ours, warmup, iters), timed(eager, warmup, iters)
    return "%-6s qp %d  n %5d   pmp_train_loss_device %8.1f us   eager torch loss + backward %8.1f us   (x%.1f)   agree: loss %.1e, gradients %.1e" % (
        comp, qp, n, t_ours, t_eager, t_eager / t_ours, dl_, dg)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--n", default="200", help="blocks per batch, comma-separated (200 is the reference's batch size)")
    ap.add_argument("--comp", default="Luma", help="Luma, Chroma or both, comma-separated")
    ap.add_argument("--qp", default=22, type=int)
    ap.add_argument("--lamb", default="", help='loss weights on top of Train_QBD\'s defaults, e.g. "lambb0=0.8,lambresb2=0"')
    ap.add_argument("--iters", default=200, type=int)
    ap.add_argument("--warmup", default=20, type=int)
    ap.add_argument("--out", default=None, help="also write the lines to this file")
    a = ap.parse_args()
    lam = engine.loss_params(a.lamb)
    if not torch.cuda.is_available():
        raise SystemExit("train_loss_bench: no GPU - there is no CPU fallback")
    eng = engine.Engine(0)
    lines = ["pmp_train_loss_device with gradients against eager torch-ROCm (loss + backward to the logits), hipEvents, %d calls after %d warm-up calls, %s"
             % (a.iters, a.warmup, torch.cuda.get_device_name(0))]
    for comp in a.comp.split(","):
        for n in a.n.split(","):
            lines.append(one(eng, comp, a.qp, int(n), lam, a.warmup, a.iters))
            print(lines[-1], flush=True)
    eng.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
