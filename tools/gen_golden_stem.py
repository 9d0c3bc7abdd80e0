"""Generate tests/golden/g18_stem_grad.npz from the IMPORTED REFERENCE: the four nets' own padding_* and conv_* modules
(Model_QBD.py:63-68, :103-110, :161-166, :201-208) in float64 with the cases' weights, under torch autograd, the way their forward
writes the first layer (:79-80, :132-135).

Run where the reference checkout is (CPU; tools/ref_harness.py sets up the path):   python tools/gen_golden_stem.py
Inputs are rebuilt by tests/stem_cases.py; only the reference's outputs are stored, per case of stem_cases.IN_GOLDEN:
  <case>/y, <case>/g_x                    the stem's output and x.grad after (y * g_y).sum().backward()
  <case>/g_w<j>, <case>/g_b<j>            the .grad of convolution j's weight and bias
Every value is an integer: stored as int8 where it fits and int32 otherwise.  A case whose (cin, k, split) is a net's runs on that
net's modules; the others (the reduction-partition cases: cin = 4 with k = 9) on the luma MTT net's padding modules and convolutions
of its kernel shapes rebuilt with the case's cin.  While generating, EVERY exact case (stored or not) must equal the functional
restatement in float64 and a float32 evaluation of it, element for element; max_abs records the largest magnitude seen.
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
import stem_cases as S  # noqa: E402

NETS = {(1, 9, 0): "Luma_Q_Net", (2, 9, 1): "Luma_MSBD_Net", (3, 5, 0): "Chroma_Q_Net", (4, 5, 1): "Chroma_MSBD_Net"}


def reference(M, c):
    """The reference's own modules in float64 -> a dict laid out like stem_cases.restate's."""
    n, h, w, cin, k, split = c["shape"]
    d = lambda a: torch.from_numpy(np.asarray(a, np.float64).copy())
    own = NETS.get((cin, k, split))
    net = getattr(M, own or {(9, 0): "Luma_Q_Net", (9, 1): "Luma_MSBD_Net", (5, 0): "Chroma_Q_Net", (5, 1): "Chroma_MSBD_Net"}[(k, split)])()
    convs = [net.conv_b1_1, net.conv_b1_2, net.conv_b1_3] if split else [net.conv_q1]
    padders = [net.padding_rb, net.padding_r, net.padding_b] if split else [net.padding_rb]
    if not own:
        convs = [torch.nn.Conv2d(cin, m.out_channels, kernel_size=m.kernel_size, padding=m.padding, stride=m.stride) for m in convs]
    convs = [m.double() for m in convs]
    with torch.no_grad():
        for m, wt, b in zip(convs, c["w"], c["b"]):
            assert tuple(m.weight.shape) == wt.shape and tuple(m.bias.shape) == b.shape, (c["shape"], m)
            m.weight.copy_(d(wt))
            m.bias.copy_(d(b))
    x = d(c["x"]).requires_grad_()
    outs = [F.relu(m(pd(x))) for m, pd in zip(convs, padders)]
    y = torch.cat(outs, 1) if split else outs[0]
    (y * d(c["g_y"])).sum().backward()
    num = lambda v: v.detach().numpy().copy()
    return {"y": num(y), "g_x": num(x.grad), "g_w": [num(m.weight.grad) for m in convs], "g_b": [num(m.bias.grad) for m in convs]}


def main():
    M = ref_harness.load()[0]
    out = {}
    biggest = 0.0
    for name in S.EXACT:
        c = S.make_case(name)
        ref, r64, r32 = S.flat(reference(M, c)), S.flat(S.restate(c, torch.float64)), S.flat(S.restate(c, torch.float32))
        assert sorted(ref) == sorted(r64) == sorted(r32), name
        for key, a in ref.items():
            assert np.array_equal(a, r64[key]), (name, key, "the reference differs from the float64 restatement")
            assert r32[key].dtype == np.float32 and np.array_equal(a, r32[key].astype(np.float64)), (name, key, "float32 is not exact")
            assert np.array_equal(a, np.rint(a)), (name, key, "not an integer")
            biggest = max(biggest, float(np.abs(a).max()))
        if name in S.IN_GOLDEN:
            for key, a in ref.items():
                out["%s/%s" % (name, key)] = a.astype(np.int8 if np.abs(a).max() <= 127 else np.int32)
        print("%-13s %-28s zeros of y: %.2f" % (name, c["shape"], float((ref["y"] == 0).mean())), flush=True)
    assert biggest < 2 ** 24, biggest
    out["max_abs"] = np.float64(biggest)
    print("largest magnitude seen: %g" % biggest)
    np.savez_compressed(S.GOLDEN, **out)
    size = os.path.getsize(S.GOLDEN)
    print("wrote", S.GOLDEN, size, "bytes")
    assert size < 1000000, size


if __name__ == "__main__":
    main()
