"""Generate tests/golden/g20_qtail_grad.npz from torch's own statements of a QT net's tail (Model_QBD.py:83-90): nn.Conv2d modules as
ResidualBlocks, F.max_pool2d, F.interpolate and torch.cat, in float64 under autograd.

Run on the CPU:   python tools/gen_golden_qtail.py
Inputs are rebuilt by tests/qtail_cases.py; only outputs are stored, per EXACT case:
  <case>/x9, <case>/g_x4                              the tail's output and x4.grad after (x9 * g_x9).sum().backward()
  <case>/g_w0_<i>, <case>/g_w2_<i>, <case>/g_wsc_<i>  the .grad of the weights of block i (0..3 = resblock_q3..q6)
Every value of the exact cases is a small integer: stored as int8 where it fits and int32 otherwise.  While generating, for EVERY
exact case autograd's results - the outputs and every intermediate the library saves - must equal the functional restatement in
float64 and a float32 evaluation of it, element for element, the ties of every pool included; max_abs records the largest sum of
|terms| any kernel can form (it must stay below 2^24).
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402
from torch import nn  # noqa: E402

import qtail_cases as Q  # noqa: E402


class ResidualBlock(nn.Module):
    def __init__(self, cin, cout, k, w0, w2, wsc):
        super().__init__()
        d = lambda a: nn.Parameter(torch.from_numpy(np.asarray(a, np.float64).copy()))
        self.c0, self.c2 = nn.Conv2d(cin, cout, k, padding=k // 2, bias=False).double(), nn.Conv2d(cout, cout, k, padding=k // 2, bias=False).double()
        self.c0.weight, self.c2.weight = d(w0), d(w2)
        self.sc = None
        if wsc is not None:
            self.sc = nn.Conv2d(cin, cout, 1, bias=False).double()
            self.sc.weight = d(wsc.reshape(cout, cin, 1, 1))

    def forward(self, x):
        self.t = F.relu(self.c0(x))
        return F.relu(self.c2(self.t) + (x if self.sc is None else self.sc(x)))


def autograd(c):
    """-> a dict laid out like qtail_cases.restate's (x9, g_x4, s, g_w)."""
    q = [ResidualBlock(ci, co, k, *blk) for (ci, co, k), blk in zip(Q.BLOCKS, c["blocks"])]
    x4 = torch.from_numpy(np.asarray(c["x4"], np.float64).copy()).requires_grad_()
    x5 = q[0](x4)
    x6 = torch.cat([x5] + [F.interpolate(F.max_pool2d(x5, s), scale_factor=s) for s in Q.SCALES], 1)
    x7 = q[1](x6)
    o5 = q[2](x7)
    x9 = q[3](F.max_pool2d(o5, 2))
    (x9 * torch.from_numpy(np.asarray(c["g_x9"], np.float64))).sum().backward()
    num = lambda v: v.detach().numpy().copy()
    return {"x9": num(x9), "g_x4": num(x4.grad), "s": [num(x4), num(q[0].t), num(x5), num(q[1].t), num(x7), num(q[2].t), num(o5), num(q[3].t), num(x9)],
            "g_w": [(num(m.c0.weight.grad), num(m.c2.weight.grad), None if m.sc is None else num(m.sc.weight.grad).reshape(m.sc.weight.shape[:2]))
                    for m in q]}


def main():
    out = {}
    biggest = 0.0
    for name in Q.EXACT:
        c = Q.make_exact(name)
        ref, r64, r32 = Q.flat(autograd(c)), Q.flat(Q.restate(c, torch.float64)), Q.flat(Q.restate(c, torch.float32))
        assert sorted(ref) == sorted(r64) == sorted(r32), name
        for key, a in ref.items():
            assert np.array_equal(a, r64[key]), (name, key, "autograd differs from the float64 restatement")
            assert r32[key].dtype == np.float32 and np.array_equal(a, r32[key].astype(np.float64)), (name, key, "float32 is not exact")
            assert np.array_equal(a, np.rint(a)), (name, key, "not an integer")
        for key in Q.golden_keys(ref):
            small = np.abs(ref[key]).max() <= 127
            out["%s/%s" % (name, key)] = ref[key].astype(np.int8 if small else np.int32)
        biggest = max(biggest, Q.worst_partial_sum(c))
        r = Q.restate(c)
        print("%-5s %-12s tied positive windows: s=2 %d, 4 %d, 8 %d, q5's pool %d" % (
            name, c["shape"], *[Q.tied_positive(r["s"][2], s) for s in Q.SCALES], Q.tied_positive(r["s"][6], 2)), flush=True)
    assert biggest < 2 ** 24, biggest
    out["max_abs"] = np.float64(biggest)
    print("largest sum of |terms|: %g" % biggest)
    np.savez_compressed(Q.GOLDEN, **out)
    size = os.path.getsize(Q.GOLDEN)
    print("wrote", Q.GOLDEN, size, "bytes")
    assert size < 1000000, size


if __name__ == "__main__":
    main()
