"""Generate tests/golden/conv5_forms.npz from a build of the library taken BEFORE a change to the 5x5 Cout-64 kernels' forms (run on the
GPU box):   python tools/gen_golden_conv5_forms.py <libpmp_hip.so of the commit before> [output .npz]

Stored (tests/test_gpu_conv5_forms.py rebuilds the inputs and compares byte for byte):
  sha256_rb.t, sha256_rb    digests of the float32 bits of RB(32,64,5) at 32x32, N = 2 (test_gpu_conv5_forms.IDENTITY_CASE): the activation
                            between the two convolutions and the block's output
  hor, ver, qt, dire        the records of one luma QP22 step of 8 blocks, as `bench.py --batch 8 --dump-outputs` writes them
"""
import os
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402


def main():
    lib = os.path.abspath(sys.argv[1])
    out = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "tests", "golden", "conv5_forms.npz")
    from pmp_vvc_tip2023_amd import _lib
    _lib.load(lib)                                   # before anything else loads the tree's own build
    import gpu_rig
    import test_gpu_conv5_forms as F
    from oracle import taps as T
    with gpu_rig.engine(threads=16, setup=lambda e: T.taps_on(e, True), poison=2) as e:
        dig = F.identity_digests(e)
    with tempfile.TemporaryDirectory() as d:
        rec = F.bench_records(os.path.join(d, "out"), lib=lib)
    np.savez_compressed(out, **{"sha256_" + k: np.array(v) for k, v in dig.items()}, **rec)
    print("wrote %s from %s: %s" % (out, lib, dig))


if __name__ == "__main__":
    main()
