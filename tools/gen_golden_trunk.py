"""Generate tests/golden/g16_trunk_grad.npz from the IMPORTED REFERENCE: Model_QBD.ResidualBlock modules in an nn.Sequential, followed
by F.max_pool2d(., 2) where the case has a pool, under torch autograd.

Run where the reference checkout is (CPU; tools/ref_harness.py sets up the path):   python tools/gen_golden_trunk.py
Inputs are rebuilt by tests/trunk_cases.py; only the reference's outputs are stored, per case of trunk_cases.IN_GOLDEN:
  <case>/y, <case>/g_x                               the trunk's output and x.grad after (y * g_y).sum().backward()
  <case>/g_w0_<i>, <case>/g_w2_<i>, <case>/g_wsc_<i>  the .grad of block i's weights
The reference runs in float64 on the exact cases, whose every value is a small integer: stored as int8 where it fits and int32
otherwise.  While generating, for EVERY exact case (stored or not) the reference - its outputs and every block's intermediate t and
output, caught by forward hooks - must equal the functional restatement in float64 and a float32 evaluation of it, element for element,
ties of the pool included; max_abs records the largest magnitude seen (it must stay below 2^24).
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, HERE)

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

import ref_harness  # noqa: E402
import trunk_cases as T  # noqa: E402


def reference(M, c):
    """The reference's own modules in float64 -> a dict laid out like trunk_cases.restate's."""
    d = lambda a: torch.from_numpy(np.asarray(a, np.float64).copy())
    mods = []
    for (cin, cout, k), (w0, w2, wsc) in zip(T.block_shapes(c["shape"]), c["blocks"]):
        rb = M.ResidualBlock(cin, cout, k, k // 2).double()
        with torch.no_grad():
            rb.left[0].weight.copy_(d(w0))
            rb.left[2].weight.copy_(d(w2))
            if wsc is not None:
                rb.shortcut[0].weight.copy_(d(wsc).reshape(cout, cin, 1, 1))
        mods.append(rb)
    seq = torch.nn.Sequential(*mods)
    ts, outs, hooks = [], [], []
    for rb in mods:
        hooks.append(rb.left[1].register_forward_hook(lambda m, i, o: ts.append(o.detach().clone())))
        hooks.append(rb.register_forward_hook(lambda m, i, o: outs.append(o.detach().clone())))
    x = d(c["x"]).requires_grad_()
    y = seq(x)
    if c["shape"][5]:
        y = F.max_pool2d(y, 2)
    for h in hooks:
        h.remove()
    (y * d(c["g_y"])).sum().backward()
    num = lambda v: v.detach().numpy().copy()
    return {"y": num(y), "g_x": num(x.grad), "t": [num(t) for t in ts], "out": [num(o) for o in outs],
            "g_w": [(num(rb.left[0].weight.grad), num(rb.left[2].weight.grad),
                     num(rb.shortcut[0].weight.grad).reshape(rb.shortcut[0].weight.shape[:2]) if len(rb.shortcut) else None) for rb in mods]}


def main():
    M = ref_harness.load()[0]
    out = {}
    biggest = 0.0
    for name in T.EXACT:
        c = T.make_exact(name)
        ref, r64, r32 = T.flat(reference(M, c)), T.flat(T.restate(c, torch.float64)), T.flat(T.restate(c, torch.float32))
        assert sorted(ref) == sorted(r64) == sorted(r32), name
        for key, a in ref.items():
            assert np.array_equal(a, r64[key]), (name, key, "the reference differs from the float64 restatement")
            assert r32[key].dtype == np.float32 and np.array_equal(a, r32[key].astype(np.float64)), (name, key, "float32 is not exact")
            assert np.array_equal(a, np.rint(a)), (name, key, "not an integer")
            biggest = max(biggest, float(np.abs(a).max()))
        if name in T.IN_GOLDEN:
            for key in T.golden_keys(ref):
                small = np.abs(ref[key]).max() <= 127
                out["%s/%s" % (name, key)] = ref[key].astype(np.int8 if small else np.int32)
        tied = T.tied_positive_windows(ref["out%d" % (len(c["blocks"]) - 1)]) if c["shape"][5] else 0
        print("%-9s %-60s tied positive pool windows: %d" % (name, c["shape"], tied), flush=True)
    assert biggest < 2 ** 24, biggest
    out["max_abs"] = np.float64(biggest)
    print("largest magnitude seen: %g" % biggest)
    np.savez_compressed(T.GOLDEN, **out)
    size = os.path.getsize(T.GOLDEN)
    print("wrote", T.GOLDEN, size, "bytes")
    assert size < 1000000, size


if __name__ == "__main__":
    main()
