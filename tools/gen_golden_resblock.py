"""Generate tests/golden/g15_resblock_grad.npz from the IMPORTED REFERENCE: Model_QBD.ResidualBlock under torch autograd.

Run where the reference checkout is (CPU; tools/ref_harness.py sets up the path):   python tools/gen_golden_resblock.py
Inputs are rebuilt by tests/resblock_cases.py; only the reference's outputs are stored, per case of resblock_cases.IN_GOLDEN (less
resblock_cases.NOT_STORED):
  <case>_t, _out                        the activation between the two convolutions (a forward hook on left[1]) and the block's output
  <case>_g_x, _g_w0, _g_w2, _g_wsc      x.grad and the weights' .grad after (out * g_out).sum().backward()
The reference runs in float64 on the exact cases, whose every value is a small integer: stored as int8 where it fits and int32
otherwise.  While generating, for EVERY exact case (stored or not) the reference must equal the functional restatement in float64 and
a float32 evaluation of it, element for element; max_abs records the largest magnitude seen (it must stay below 2^24).
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
import resblock_cases as K  # noqa: E402


def reference(M, c):
    """The reference's own module in float64 -> dict over K.OUTPUTS."""
    n, h, w, cin, cout, k = c["shape"]
    rb = M.ResidualBlock(cin, cout, k, k // 2).double()
    d = lambda a: torch.from_numpy(np.asarray(a, np.float64).copy())
    with torch.no_grad():
        rb.left[0].weight.copy_(d(c["w0"]))
        rb.left[2].weight.copy_(d(c["w2"]))
        if c["wsc"] is not None:
            rb.shortcut[0].weight.copy_(d(c["wsc"]).reshape(cout, cin, 1, 1))
    seen = {}
    hook = rb.left[1].register_forward_hook(lambda m, i, o: seen.__setitem__("t", o.detach().clone()))
    x = d(c["x"]).requires_grad_()
    out = rb(x)
    hook.remove()
    (out * d(c["g_out"])).sum().backward()
    r = {"t": seen["t"], "out": out.detach(), "g_x": x.grad, "g_w0": rb.left[0].weight.grad, "g_w2": rb.left[2].weight.grad,
         "g_wsc": rb.shortcut[0].weight.grad.reshape(cout, cin) if c["wsc"] is not None else None}
    return {k: None if v is None else v.numpy().copy() for k, v in r.items()}


def main():
    M = ref_harness.load()[0]
    out = {}
    biggest = 0.0
    for name in K.EXACT:
        c = K.make_exact(name)
        ref, r64, r32 = reference(M, c), K.restate(c, torch.float64), K.restate(c, torch.float32)
        pos = []
        for key in K.OUTPUTS:
            if ref[key] is None:
                assert r64[key] is None and r32[key] is None, (name, key)
                continue
            assert np.array_equal(ref[key], r64[key]), (name, key, "the reference differs from the float64 restatement")
            assert r32[key].dtype == np.float32 and np.array_equal(ref[key], r32[key].astype(np.float64)), (name, key, "float32 is not exact")
            assert np.array_equal(ref[key], np.rint(ref[key])), (name, key, "not an integer")
            biggest = max(biggest, float(np.abs(ref[key]).max()))
            if key in ("t", "out"):
                pos.append(float((ref[key] > 0).mean()))
                assert (ref[key] == 0).any(), (name, key, "no exact zero")
            if name in K.IN_GOLDEN and (name, key) not in K.NOT_STORED:
                small = np.abs(ref[key]).max() <= 127
                out["%s_%s" % (name, key)] = ref[key].astype(np.int8 if small else np.int32)
        print("%-12s %-24s positive share of t, out: %.2f %.2f" % (name, c["shape"], pos[0], pos[1]), flush=True)
    assert biggest < 2 ** 24, biggest
    out["max_abs"] = np.float64(biggest)
    print("largest magnitude seen: %g" % biggest)
    np.savez_compressed(K.GOLDEN, **out)
    size = os.path.getsize(K.GOLDEN)
    print("wrote", K.GOLDEN, size, "bytes")
    assert size < 1000000, size


if __name__ == "__main__":
    main()
