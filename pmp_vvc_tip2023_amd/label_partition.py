"""PartitionMat files from VTM's own partition labels: GenMSBtMap.get_sequence_partition_for_VTM on the GPU, from decoder dumps.

    python -m pmp_vvc_tip2023_amd.label_partition --depthDir DepthSaving/ --seqTable Sequences.txt --outDir Out/ \\
           [--qps 22,27,32,37] [--comps Luma,Chroma] [--ssRatio 8] [--binary] [--chromaFactor fn|1|2] [--keepFlagged]

Such a file is a perfect predictor's: fed to the patched VTM encoder it gives the ceiling of speed-up and BD-rate that the map
representation allows, and it needs no trained net.
The sequence table and the dumps are gen_labels' (same rows, same two dump names, ceil(frames / ssRatio) frames each).  For every
(sequence, component, QP) the dump is parsed (pmp_read_depth_dump, host), qtDepth - 1 is formed on the u8 array as
GenMSBtMap.main_process does (:477), the split flags are painted on the GPU (pmp_label_partition) and the existing writers emit
    <outDir>/PartitionMat/<seq>_<Luma|Chroma>_QP<qp>_PartitionMat.txt      (or .pmpb with --binary)
with the labels themselves as the file's qt and direction sections (GenMSBtMap.py:407-408).  A direction of -1 is written as -1; the
reference prints 255 there (a u8 cast, :413), which VTM's int8_t reads back as -1.
--chromaFactor: fn (default) paints Chroma with chroma factor 2, as get_sequence_partition_for_VTM's is_luma=False does; 2 is the
same; 1 paints both components with factor 1, the factor gen_labels' default labels were made with.
A sequence with a flagged block - status bit 2 (a qt value above 3) or 4 (leaf budget), include/pmp.h: pmp_label_partition - gets no
file and makes the tool exit with status 3, unless --keepFlagged is given.  Bad flags, missing or malformed dumps and sequences
smaller than one 64x64 block stop it with status 2 before any GPU work: every dump is parsed first.
"""
import argparse
import os
import sys

import numpy as np

from . import _lib
from . import engine as E
from . import gen_labels as G


def build_parser():
    p = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    p.add_argument("--depthDir", required=True, help="directory of the Save_Depth_fal dumps")
    p.add_argument("--seqTable", required=True, help="sequence table (name,file,W,H,frames[,fps] per line)")
    p.add_argument("--outDir", required=True)
    p.add_argument("--qps", default="22,27,32,37")
    p.add_argument("--comps", default="Luma,Chroma")
    p.add_argument("--ssRatio", default=8, type=int, help="temporal sub-sampling of the dumped frames (CreateDataSet.py:292)")
    p.add_argument("--binary", action="store_true", help="write the PMPB1 binary side channel (.pmpb) instead of text")
    p.add_argument("--chromaFactor", default="fn", choices=["fn", "1", "2"])
    p.add_argument("--keepFlagged", action="store_true", help="exit 0 and write the file even where status bit 2 or 4 is set")
    p.add_argument("--device", default=0, type=int)
    return p


def read_dumps(seqs, comps, qps, dumps):
    """Parses every dump on the host -> {(comp, qp, name): (qt8, bt, dire, unknown codes)}.  SystemExit(2) on a dump the parser refuses
    or a sequence without a single block."""
    def fail(msg):
        print("label_partition: " + msg, file=sys.stderr)
        raise SystemExit(2)
    for name, w, h, f in seqs:
        if f * (h // 64) * (w // 64) <= 0:
            fail("sequence %s (%dx%d, %d frames) holds no 64x64 block" % (name, w, h, f))
    out = {}
    for comp in comps:
        for qp in qps:
            for name, w, h, f in seqs:
                path = dumps[(comp, qp, name)]
                try:
                    out[(comp, qp, name)] = E.output_block_partition_map(path, w, h, f, 64, comp == "Chroma", return_unknown=True)
                except _lib.PmpError as e:
                    fail("%s: %s" % (path, e))
    return out


def main(argv=None):
    args = build_parser().parse_args(argv)
    qps, comps, seqs, dumps = G.plan(args, tool="label_partition")
    blocks = read_dumps(seqs, comps, qps, dumps)
    out_dir = os.path.join(args.outDir, "PartitionMat")
    os.makedirs(out_dir, exist_ok=True)
    eng = E.Engine(args.device)
    refused = 0
    try:
        for comp in comps:
            cf = 1 if (comp == "Luma" or args.chromaFactor == "1") else 2
            for qp in qps:
                for name, w, h, f in seqs:
                    qt8, bt, dire, unknown = blocks.pop((comp, qp, name))
                    path = os.path.join(out_dir, "%s_%s_QP%d_PartitionMat.%s" % (name, comp, qp, "pmpb" if args.binary else "txt"))
                    qt = qt8 - np.uint8(1)                                   # GenMSBtMap.py:477, a u8 subtraction
                    hor, ver, st = eng.label_partition(qt, bt, dire, cf)
                    counts = {bit: int(np.count_nonzero(st & bit)) for bit in (2, 4)}
                    print("%s %s QP%d: %d blocks, cf %d, unknown split codes %d; status bit2 (qt > 3) %d, bit4 (leaf budget) %d"
                          % (name, comp, qp, len(qt), cf, unknown, counts[2], counts[4]))
                    if st.any() and not args.keepFlagged:
                        print("%s %s QP%d: %s not written (--keepFlagged writes it)" % (name, comp, qp, path), file=sys.stderr)
                        refused += 1
                        continue
                    (E.write_partition_binary if args.binary else E.write_partition_file)(path, f, h, w, hor, ver, qt, dire)
    finally:
        eng.close()
    return 3 if refused else 0


if __name__ == "__main__":
    sys.exit(main())
