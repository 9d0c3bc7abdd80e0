"""Generate tests/golden/g21_dataset.npz from the IMPORTED REFERENCE: CreateDataSet.output_block_yuv, the block side of its data sets.

Run where the reference checkout is (the module imports pyplot):   MPLBACKEND=Agg python tools/gen_golden_dataset.py
The input is rebuilt by tests/dataset_cases.py (G21: 192x136, 33 frames, SubSampleRatio 8, 8 and 10 bits); only outputs are stored:
  by8, bu8, bv8, by10, bu10, bv10     output_block_yuv(file, 192, 136, 64, 4, 33, 8, is10bit): u8[30,68,68], u8[30,34,34] twice
"""
import contextlib
import io
import os
import sys
import tempfile
import warnings

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(ROOT, "tests"))
os.environ.setdefault("MPLBACKEND", "Agg")

import numpy as np  # noqa: E402

import dataset_cases as K  # noqa: E402

REF = os.environ.get("PMP_REFERENCE_DIR", "/root/reference")


def main():
    sys.dont_write_bytecode = True
    if REF not in sys.path:
        sys.path.insert(0, REF)
    import CreateDataSet as CD
    g, out = K.G21, {}
    with tempfile.TemporaryDirectory() as d, warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for bits in (8, 10):
            path = os.path.join(d, "seq%d.yuv" % bits)
            K.write_yuv(path, g["width"], g["height"], g["frames"], bits, g["seed"])
            with contextlib.redirect_stdout(io.StringIO()):
                by, bu, bv = CD.output_block_yuv(path, g["width"], g["height"], 64, 4, g["frames"], g["ss"], is10bit=bits == 10)
            out["by%d" % bits], out["bu%d" % bits], out["bv%d" % bits] = by, bu, bv
            print(bits, "bits:", by.shape, bu.shape, bv.shape, by.dtype)
    np.savez_compressed(K.GOLDEN, **out)
    print("wrote", K.GOLDEN, os.path.getsize(K.GOLDEN), "bytes")


if __name__ == "__main__":
    main()
