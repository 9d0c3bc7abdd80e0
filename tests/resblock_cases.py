"""Cases and a float64 restatement of one Model_QBD.ResidualBlock, forward and backward (include/pmp.h: pmp_resblock_forward /
pmp_resblock_backward; csrc/api_train.cpp, conv_wgrad.hip).  Shared by tests/test_resblock_cases_cpu.py, tests/test_gpu_resblock_grad.py
and tools/gen_golden_resblock.py; inputs are rebuilt from a per-case seed, only the reference's outputs are stored in the golden.

EXACT cases.  x uniform integers in [-2, 2], every weight and the upstream gradient in {-1, 0, 1}.  Every intermediate and every
gradient is then an integer, and worst_partial_sum() gives, per case, the largest sum of the MAGNITUDES of the terms of any output
element (each operation on the absolute values of its actual inputs): below 2^24 (tests/test_resblock_cases_cpu.py), so every partial
sum in ANY order of summation is an integer that float32 holds exactly, and a float32 kernel must equal the float64 result bit for
bit, no element left out.  About half of t and out are positive
and exact zeros occur, which exercises the `> 0` rule of the masks.

FLOAT cases.  Normal x and g_out, normal weights scaled by 1 / sqrt(fan-in).  t and out are handed to the backward pass as the float32
roundings of a float64 forward, so the masks are the same for every implementation and nothing needs to be excluded.
"""
import os

import numpy as np
import torch
import torch.nn.functional as F

from cases_common import as_f32, same_bits  # noqa: F401 (K.as_f32, K.same_bits)

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g15_resblock_grad.npz")
OUTPUTS = ("t", "out", "g_x", "g_w0", "g_w2", "g_wsc")

# name -> (n, h, w, cin, cout, k)
EXACT = {
    "identity":   (2, 16, 16, 16, 16, 3),     # identity shortcut
    "sc_5x5":     (2, 32, 32, 32, 64, 5),     # conv shortcut; halos across tile borders
    "c64_5x5":    (2, 32, 32, 64, 64, 5),     # the largest accumulator set
    "c64_32":     (2, 32, 32, 64, 32, 3),
    "padded_cin": (3, 16, 48, 3, 32, 3),      # padded cin, non-square, odd n
    "padded_cout": (2, 16, 16, 16, 8, 3),     # padded cout
    "prime_n":    (37, 16, 16, 16, 16, 3),    # a prime n: crosses whatever partition the partial sums use
    # 144 work items on 4 input groups: the weight gradients of w0 and wsc run at their cap of 64 partial sums, 16 workgroups adding
    # three tiles and 48 adding two (an uneven tail); w2's (one group) at 72 partial sums of two tiles
    "many_tiles": (9, 64, 64, 64, 16, 3),
}
IN_GOLDEN = ("identity", "sc_5x5", "padded_cout", "prime_n")      # the 16x16 cases and (2,32,32,32,64,5)
# ... less one tensor, to keep the file below 1 MB: prime_n is there for the partition of the weight gradients' partial sums, and its
# g_x (a per-pixel result, 200 kB compressed) is checked against the reference when the golden is generated, like the cases not stored
NOT_STORED = {("prime_n", "g_x")}
FLOAT = {
    "f_sc_5x5": (2, 32, 32, 32, 64, 5),
    "f_c64_32": (4, 16, 16, 64, 32, 3),
}


def _seed(name):
    return 20231 + sum((i + 1) * ord(ch) for i, ch in enumerate(name))


def make_exact(name):
    """-> dict(shape, x, w0, w2, wsc or None, g_out) as float32 numpy arrays of small integers."""
    n, h, w, cin, cout, k = EXACT[name]
    g = torch.Generator().manual_seed(_seed(name))
    ri = lambda lo, hi, *s: torch.randint(lo, hi + 1, s, generator=g).to(torch.float32).numpy()
    c = {"shape": EXACT[name], "x": ri(-2, 2, n, cin, h, w), "w0": ri(-1, 1, cout, cin, k, k), "w2": ri(-1, 1, cout, cout, k, k)}
    c["wsc"] = ri(-1, 1, cout, cin) if cin != cout else None
    c["g_out"] = ri(-1, 1, n, cout, h, w)
    return c


def make_float(name):
    """-> the same with normal values; weights scaled by 1 / sqrt(fan-in)."""
    n, h, w, cin, cout, k = FLOAT[name]
    g = torch.Generator().manual_seed(_seed(name))
    rn = lambda scale, *s: (torch.randn(s, generator=g, dtype=torch.float64) * scale).to(torch.float32).numpy()
    c = {"shape": FLOAT[name], "x": rn(1.0, n, cin, h, w), "w0": rn((cin * k * k) ** -0.5, cout, cin, k, k),
         "w2": rn((cout * k * k) ** -0.5, cout, cout, k, k)}
    c["wsc"] = rn(cin ** -0.5, cout, cin) if cin != cout else None
    c["g_out"] = rn(1.0, n, cout, h, w)
    return c


def _t(a, dtype):
    return None if a is None else torch.as_tensor(np.asarray(a)).to(dtype)


def forward(x, w0, w2, wsc=None, dtype=torch.float64):
    """t = relu(conv0(x)), out = relu(conv2(t) + sc(x)) in `dtype` on the CPU -> (t, out) numpy arrays of that dtype."""
    x, w0, w2, wsc = _t(x, dtype), _t(w0, dtype), _t(w2, dtype), _t(wsc, dtype)
    p = w0.shape[2] // 2
    t = F.relu(F.conv2d(x, w0, padding=p))
    sc = x if wsc is None else F.conv2d(x, wsc.reshape(wsc.shape[0], wsc.shape[1], 1, 1))
    out = F.relu(F.conv2d(t, w2, padding=p) + sc)
    return t.numpy(), out.numpy()


def backward(x, t, out, w0, w2, wsc, g_out, dtype=torch.float64, want_g_x=True):
    """The formulas of include/pmp.h, term for term, in `dtype` on the CPU -> dict(g_x, g_w0, g_w2, g_wsc) (None where absent)."""
    x, t, out, w0, w2, wsc, g = (_t(a, dtype) for a in (x, t, out, w0, w2, wsc, g_out))
    p = w0.shape[2] // 2
    zero = torch.zeros((), dtype=dtype)
    gu = torch.where(out > 0, g, zero)
    r = {"g_w2": torch.nn.grad.conv2d_weight(t, w2.shape, gu, padding=p), "g_wsc": None, "g_x": None}
    wsc4 = None if wsc is None else wsc.reshape(wsc.shape[0], wsc.shape[1], 1, 1)
    if wsc is not None:
        r["g_wsc"] = torch.nn.grad.conv2d_weight(x, wsc4.shape, gu).reshape(wsc.shape)
    gt = torch.where(t > 0, F.conv_transpose2d(gu, w2, padding=p), zero)
    r["g_w0"] = torch.nn.grad.conv2d_weight(x, w0.shape, gt, padding=p)
    if want_g_x:
        r["g_x"] = F.conv_transpose2d(gt, w0, padding=p) + (gu if wsc is None else F.conv_transpose2d(gu, wsc4))
    return {k: None if v is None else v.numpy() for k, v in r.items()}


def restate(c, dtype=torch.float64):
    """Forward and backward of a case -> dict over OUTPUTS."""
    t, out = forward(c["x"], c["w0"], c["w2"], c["wsc"], dtype)
    r = backward(c["x"], t, out, c["w0"], c["w2"], c["wsc"], c["g_out"], dtype)
    r["t"], r["out"] = t, out
    return r


def worst_partial_sum(c):
    """The largest sum of |term| over the output elements of every operation of a case, each on the magnitudes of its actual inputs:
    a bound on every partial sum a kernel can form, whatever its order."""
    d = torch.float64
    r = restate(c)
    a = lambda v: None if v is None else _t(np.abs(v), d)
    x, w0, w2, wsc, g, t = a(c["x"]), a(c["w0"]), a(c["w2"]), a(c["wsc"]), a(c["g_out"]), a(r["t"])
    p = w0.shape[2] // 2
    wsc4 = None if wsc is None else wsc.reshape(wsc.shape[0], wsc.shape[1], 1, 1)
    gu = torch.where(_t(r["out"], d) > 0, g, torch.zeros((), dtype=d))
    gt = a(np.where(r["t"] > 0, F.conv_transpose2d(_t(np.where(r["out"] > 0, c["g_out"], 0), d), _t(c["w2"], d), padding=p).numpy(), 0))
    sums = [F.conv2d(x, w0, padding=p), F.conv2d(t, w2, padding=p) + (x if wsc is None else F.conv2d(x, wsc4)),
            torch.nn.grad.conv2d_weight(t, w2.shape, gu, padding=p), F.conv_transpose2d(gu, w2, padding=p),
            torch.nn.grad.conv2d_weight(x, w0.shape, gt, padding=p),
            F.conv_transpose2d(gt, w0, padding=p) + (gu if wsc is None else F.conv_transpose2d(gu, wsc4))]
    if wsc is not None:
        sums.append(torch.nn.grad.conv2d_weight(x, wsc4.shape, gu))
    return max(float(v.max()) for v in sums)


def rel_err(a, ref64):
    """E = max |a - ref| / max |ref| of one tensor."""
    ref64 = np.asarray(ref64, np.float64)
    return float(np.abs(np.asarray(a, np.float64) - ref64).max() / np.abs(ref64).max())
