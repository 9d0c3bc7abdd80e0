"""Generate tests/golden/g11_msbt.npz from the IMPORTED REFERENCE: GenMSBtMap labels and CreateDataSet's dump parser.

Run where the reference checkout is (both modules import pyplot):   MPLBACKEND=Agg python tools/gen_golden_msbt.py
Inputs are rebuilt by tests/msbt_cases.py; only outputs are stored:
  <case>_msbt u8[n,3,16,16], <case>_raised bool[n]   GenMSBtMap.getSubMap(qt, bt, dire, cf) per block (zeros where it raised)
  wrap_idx                                            blocks of the wrap pool whose result changes when bt is int16 instead of u8
  dump_<name>_{qt,bt,dire}, dump_<name>_unknown      CreateDataSet.output_block_partition_map on msbt_cases.DUMPS, and its
                                                      count of "Error!!" lines
  pipe_<comp>_<qp>_{qt,bt,dire,msbt}                  save_partition_block_set + GenMSBtMap.main_process on msbt_cases.write_pipe_dir
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

import msbt_cases as K  # noqa: E402

REF = os.environ.get("PMP_REFERENCE_DIR", "/root/reference")


def _ref():
    sys.dont_write_bytecode = True
    if REF not in sys.path:
        sys.path.insert(0, REF)
    import CreateDataSet
    import GenMSBtMap
    return CreateDataSet, GenMSBtMap


def sub_maps(G, qt, bt, dire, cf):
    out = np.zeros((len(qt), 3, 16, 16), np.uint8)
    raised = np.zeros(len(qt), bool)
    for i in range(len(qt)):
        try:
            out[i] = G.getSubMap(qt[i], bt[i], dire[i], cf)
        except AttributeError:          # best leaf above depth 3 (GenMSBtMap.py:342-349)
            raised[i] = True
    return out, raised


def parse_dump(CD, text, frames, height, width, chroma):
    with tempfile.TemporaryDirectory() as d:
        p = os.path.join(d, "dump.txt")
        with open(p, "w") as fp:
            fp.write(text)
        buf = io.StringIO()
        with contextlib.redirect_stdout(buf):
            q, b, r = CD.output_block_partition_map(p, width, height, frames, block_size=64, isChroma=chroma)
    return q, b, r, buf.getvalue().count("Error!!")


def main():
    CD, G = _ref()
    out = {}
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for name, cf, (qt, bt, dire) in K.label_sets():
            m, r = sub_maps(G, qt, bt, dire, cf)
            out[name + "_msbt"], out[name + "_raised"] = m, r
            print(name, len(qt), "blocks,", int(r.sum()), "raised", flush=True)
            if name == "wrap":
                m16, r16 = sub_maps(G, qt, bt.astype(np.int16), dire, cf)
                diff = (r != r16) | np.any(m != m16, axis=(1, 2, 3))
                out["wrap_idx"] = np.nonzero(diff)[0].astype(np.int32)
                print("wrap: %d of %d blocks change with int16 labels" % (len(out["wrap_idx"]), len(qt)))
        for (name, seed, fw, frames, h, w, chroma, rate) in K.DUMPS:
            q, b, r, unk = parse_dump(CD, K.make_dump(seed, fw, h, w, chroma, rate), frames, h, w, chroma)
            out["dump_%s_qt" % name], out["dump_%s_bt" % name], out["dump_%s_dire" % name] = q, b, r
            out["dump_%s_unknown" % name] = np.int64(unk)
            print("dump", name, q.shape, "unknown", unk)
        with tempfile.TemporaryDirectory() as d:
            K.write_pipe_dir(d)
            for comp in ("Luma", "Chroma"):
                for qp in K.PIPE_QPS:
                    qs, bs, ds = [], [], []
                    for (name, w, h, f) in K.PIPE_SEQS:
                        path = [os.path.join(d, "%s_QP%d_%s%s" % (name, qp, comp, s))
                                for s in ("_Partition.txt", "_Partition_FastOff_LFNST0.txt")]
                        path = [p for p in path if os.path.isfile(p)][0]
                        q, b, r, _ = parse_dump(CD, open(path).read(), (f + K.PIPE_SS - 1) // K.PIPE_SS, h, w, comp == "Chroma")
                        qs.append(q); bs.append(b); ds.append(r)
                    q, b, r = np.concatenate(qs), np.concatenate(bs), np.concatenate(ds)
                    with contextlib.redirect_stdout(io.StringIO()):
                        m = G.gen_seq_sub_map(qt_map=q - 1, bt_map=b, dire_map=r, is_luma=True)   # GenMSBtMap.py:477-483
                    key = "pipe_%s_%d_" % (comp, qp)
                    out[key + "qt"], out[key + "bt"], out[key + "dire"], out[key + "msbt"] = q, b, r, m
                    print("pipe", comp, qp, q.shape)
    np.savez_compressed(K.GOLDEN, **out)
    print("wrote", K.GOLDEN, os.path.getsize(K.GOLDEN), "bytes")


if __name__ == "__main__":
    main()
