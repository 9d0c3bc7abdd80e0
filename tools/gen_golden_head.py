"""Generate tests/golden/g19_head_grad.npz from the reference's own statements for an MTT net's head (Model_QBD.py:139-153): an
nn.Conv2d(cin, cout, kernel_size=3, padding=1, stride=1) as the nets declare conv_B1..3, the in-place carry
out[:, 0:1] = out[:, 0:1] + prev[:, 0:1], F.interpolate(., scale_factor=) and torch.cat, in float64 under torch autograd.

Run on the CPU:   python tools/gen_golden_head.py
Inputs are rebuilt by tests/head_cases.py; only the outputs are stored, per case of head_cases.IN_GOLDEN:
  <case>/y, <case>/att                    the carried head output and the next attention trunk's input
  <case>/g_x, g_w, g_b, g_q, g_prev       the .grad of x, the convolution's weight and bias, q and prev after
                                          ((y * g_y).sum() + (att * g_att).sum()).backward()
(att, g_q only with an attention input, g_prev only with a carry.)  Every value is an integer: stored as int8 where it fits and int32
otherwise.  While generating, EVERY exact case (stored or not) must equal the numpy restatement element for element.
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

import head_cases as H  # noqa: E402


def reference(c):
    n, h, w, cin, cout, up_q, up_y = c["shape"]
    d = lambda a: None if a is None else torch.from_numpy(np.asarray(a, np.float64).copy())
    conv = torch.nn.Conv2d(cin, cout, kernel_size=3, padding=1, stride=1).double()
    with torch.no_grad():
        conv.weight.copy_(d(c["w"]))
        conv.bias.copy_(d(c["b"]))
    x = d(c["x"]).requires_grad_()
    prev = None if c["prev"] is None else d(c["prev"]).requires_grad_()
    q = None if c["q"] is None else d(c["q"]).requires_grad_()
    out = conv(x)
    if prev is not None:
        out[:, 0:1, :, :] = out[:, 0:1, :, :] + prev[:, 0:1, :, :]
    loss = (out * d(c["g_y"])).sum()
    att = None
    if up_y:
        att = torch.cat([F.interpolate(q, scale_factor=up_q), F.interpolate(out, scale_factor=up_y) if up_y > 1 else out], 1)
        loss = loss + (att * d(c["g_att"])).sum()
    loss.backward()
    num = lambda v: None if v is None else v.detach().numpy().copy()
    return {"y": num(out), "att": num(att), "g_x": num(x.grad), "g_w": num(conv.weight.grad), "g_b": num(conv.bias.grad),
            "g_q": None if q is None else num(q.grad), "g_prev": None if prev is None else num(prev.grad)}


def main():
    out = {}
    biggest = 0.0
    for name in H.EXACT:
        c = H.make_case(name)
        ref, r64 = reference(c), H.restate(c)
        if c["prev"] is None:
            r64["g_prev"] = None
        assert sorted(ref) == sorted(r64), name
        for key, a in ref.items():
            assert (a is None) == (r64[key] is None), (name, key)
            if a is None:
                continue
            assert np.array_equal(a, r64[key]), (name, key, "the reference's statements differ from the restatement")
            assert np.array_equal(a, np.rint(a)), (name, key, "not an integer")
            biggest = max(biggest, float(np.abs(a).max()))
            if name in H.IN_GOLDEN:
                out["%s/%s" % (name, key)] = a.astype(np.int8 if np.abs(a).max() <= 127 else np.int32)
        print("%-10s %s" % (name, c["shape"]), flush=True)
    assert biggest < 2 ** 24, biggest
    out["max_abs"] = np.float64(biggest)
    np.savez_compressed(H.GOLDEN, **out)
    size = os.path.getsize(H.GOLDEN)
    print("largest magnitude seen: %g; wrote %s, %d bytes" % (biggest, H.GOLDEN, size))
    assert size < 100000, size


if __name__ == "__main__":
    main()
