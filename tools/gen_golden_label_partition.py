"""Generate tests/golden/g13_label_partition.npz from the IMPORTED REFERENCE: GenMSBtMap.map_to_parititon and the PartitionMat files of
GenMSBtMap.get_sequence_partition_for_VTM.

Run where the reference checkout is (PMP_REFERENCE_DIR; GenMSBtMap imports pyplot):   MPLBACKEND=Agg python tools/gen_golden_label_partition.py
Inputs are rebuilt by tests/msbt_cases.py (through tests/label_partition_cases.py); only outputs are stored:
  <set>_hor, <set>_ver u8[n,16,16]     map_to_parititon(qt, bt, dire, cf) per block, for every set of label_partition_cases.label_sets()
                                       (it finishes and raises on none of them)
  file_<seq>_<comp>_<qp>_text u8[..]   the bytes of the file get_sequence_partition_for_VTM writes for each sequence of
                                       msbt_cases.write_pipe_dir (dump -> CreateDataSet.output_block_partition_map -> qtDepth - 1 on u8,
                                       is_luma = (comp == "Luma")), exactly as written: -1 directions appear as 255 there
That function indexes frame 2 for its plot after closing the file; on these 1- and 2-frame sequences it raises IndexError, which is
caught: the file is complete by then.
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
sys.path.insert(0, HERE)
os.environ.setdefault("MPLBACKEND", "Agg")

import numpy as np  # noqa: E402

import gen_golden_msbt as M  # noqa: E402
import label_partition_cases as LP  # noqa: E402


def main():
    CD, G = M._ref()
    out = {}
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for name, cf, (qt, bt, dire) in LP.label_sets():
            hv = [G.map_to_parititon(qt[i], bt[i], dire[i], cf) for i in range(len(qt))]
            out[name + "_hor"] = np.stack([h for h, _ in hv]).astype(np.uint8)
            out[name + "_ver"] = np.stack([v for _, v in hv]).astype(np.uint8)
            print(name, len(qt), "blocks", flush=True)
        with tempfile.TemporaryDirectory() as d:
            LP.K.write_pipe_dir(d)
            for seq, comp, qp, w, h, frames in LP.pipe_cases():
                q, b, r, _ = M.parse_dump(CD, open(LP.pipe_dump_path(d, seq, comp, qp)).read(), frames, h, w, comp == "Chroma")
                path = os.path.join(d, "out.txt")
                with contextlib.redirect_stdout(io.StringIO()):
                    try:
                        G.get_sequence_partition_for_VTM(q - 1, b, r, comp == "Luma", path, frames, w, h)
                    except IndexError:      # check_frm_id = 2 (GenMSBtMap.py:427-428), after out_file.close()
                        pass
                out[LP.pipe_key(seq, comp, qp) + "text"] = np.frombuffer(open(path, "rb").read(), np.uint8)
                print("file", seq, comp, qp, out[LP.pipe_key(seq, comp, qp) + "text"].size, "bytes", flush=True)
    np.savez_compressed(LP.GOLDEN, **out)
    print("wrote", LP.GOLDEN, os.path.getsize(LP.GOLDEN), "bytes")


if __name__ == "__main__":
    main()
