"""Generate tests/golden/g17_grad_sweep.npz from the IMPORTED REFERENCE: Model_QBD.ResidualBlock under torch autograd, alone and in an
nn.Sequential with F.max_pool2d, on the cases of tests/grad_cases.py - the ground tests/golden/g15 and g16 do not cover: 5x5 layers with
16 or 32 padded channels, ragged channel counts, eight blocks.

Run where the reference checkout is (CPU; tools/ref_harness.py sets up the path):   python tools/gen_golden_grad_sweep.py
Inputs are rebuilt by tests/grad_cases.py; only the reference's outputs are stored:
  <case>/g_x, /g_w0, /g_w2, /g_wsc                 of the block cases grad_cases.IN_GOLDEN_BLOCKS
  <case>/y, /g_x, /g_w0_<i>, /g_w2_<i>, /g_wsc_<i>  of the trunk cases grad_cases.IN_GOLDEN_TRUNKS
as int8 where they fit and int32 otherwise.  While generating, EVERY exact block case and EVERY trunk case of the table (stored or not)
must equal the float64 restatement element for element, saved activations included; max_abs records the largest magnitude seen.
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, os.path.join(ROOT, "tests"), HERE):
    sys.path.insert(0, p)

import numpy as np  # noqa: E402

import gen_golden_resblock  # noqa: E402
import gen_golden_trunk  # noqa: E402
import grad_cases as G  # noqa: E402
import ref_harness  # noqa: E402
import resblock_cases as K  # noqa: E402
import trunk_cases as T  # noqa: E402


def main():
    M = ref_harness.load()[0]
    out = {}
    biggest = 0.0

    def store(key, a):
        out[key] = a.astype(np.int8 if np.abs(a).max() <= 127 else np.int32)

    for name in G.BLOCKS:
        c = G.make_block(name)
        ref, r64 = gen_golden_resblock.reference(M, c), K.restate(c)
        for key in K.OUTPUTS:
            if ref[key] is None:
                assert r64[key] is None, (name, key)
                continue
            assert np.array_equal(ref[key], r64[key]), (name, key, "the reference differs from the float64 restatement")
            assert np.array_equal(ref[key], np.rint(ref[key])), (name, key, "not an integer")
            biggest = max(biggest, float(np.abs(ref[key]).max()))
            if name in G.IN_GOLDEN_BLOCKS and key.startswith("g_"):
                store("%s/%s" % (name, key), ref[key])
        print("%-14s %s" % (name, c["shape"]), flush=True)
    for name in G.TRUNKS:
        c, r64 = G.trunk_exact(name)
        ref = T.flat(gen_golden_trunk.reference(M, c))
        assert sorted(ref) == sorted(r64), name
        for key, a in ref.items():
            assert np.array_equal(a, r64[key]), (name, key, "the reference differs from the float64 restatement")
            assert np.array_equal(a, np.rint(a)), (name, key, "not an integer")
            biggest = max(biggest, float(np.abs(a).max()))
        if name in G.IN_GOLDEN_TRUNKS:
            for key in T.golden_keys(ref):
                store("%s/%s" % (name, key), ref[key])
        print("%-14s %s" % (name, c["shape"]), flush=True)
    assert biggest < 2 ** 24, biggest
    out["max_abs"] = np.float64(biggest)
    print("largest magnitude seen: %g" % biggest)
    np.savez_compressed(G.GOLDEN, **out)
    size = os.path.getsize(G.GOLDEN)
    print("wrote", G.GOLDEN, size, "bytes")
    assert size < 1000000, size


if __name__ == "__main__":
    main()
