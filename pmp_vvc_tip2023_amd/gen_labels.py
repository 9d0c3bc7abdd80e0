"""MTT-net training labels from VTM partition dumps: CreateDataSet.save_partition_block_set + GenMSBtMap.main_process on the GPU.

    python -m pmp_vvc_tip2023_amd.gen_labels --depthDir DepthSaving/ --seqTable Training_Sequences.txt --outDir Label/ \\
           [--qps 22,27,32,37] [--comps Luma,Chroma] [--ssRatio 8] [--dataType Train] [--chromaFactor ref|1|2] [--keepInconsistent]

For every (component, QP), the dumps of all sequences of the table (rows `name,file,W,H,frames[,fps]`, up to a line containing
'end!!!!'; ceil(frames / ssRatio) frames each, CreateDataSet.py:290-294) are parsed (pmp_read_depth_dump, host) and concatenated in
table order, then labelled on the GPU (pmp_msbt_labels).  A dump is <depthDir>/<seq>_QP<qp>_<comp>_Partition.txt (CreateDataSet.py:301)
or DecLib's own name <seq>_QP<qp>_<comp>_Partition_FastOff_LFNST0.txt (DecLib.cpp:1019-1020).  Written to --outDir, the reference's
names and dtypes:
    <dataType>_<comp>_QP<qp>_QTdepth_Block8.npy      u8[n,8,8]      raw qtDepth, as CreateDataSet saves it
    <dataType>_<comp>_QP<qp>_BTdepth_Block16.npy     u8[n,16,16]
    <dataType>_<comp>_QP<qp>_MSdirection_Block16.npy i8[n,3,16,16]
    <dataType>_<comp>_QP<qp>_MSBTdepth_Block16.npy   u8[n,3,16,16]  from qtDepth - 1 (a u8 subtraction, GenMSBtMap.py:477)
    <dataType>_<comp>_QP<qp>_MSBTstatus.npy          u8[n]          status bits (include/pmp.h: pmp_msbt_labels)
--chromaFactor: ref (default) labels both components with chroma factor 1, as main_process does (GenMSBtMap.py:483 passes
is_luma=True for both); 1 is the same; 2 gives Chroma the factor 2 that gen_seq_sub_map's is_luma=False would.
Blocks with status bit 1 (the reference raises on them) or 4 (leaf budget) make the tool exit with status 3 after writing everything
but their pair's MSBTdepth file, unless --keepInconsistent is given.  A missing dump or a bad flag stops it before any GPU work.
"""
import argparse
import os
import sys

import numpy as np

from . import engine as E
from .inference_qbd import load_sequences_info

COMPS = ("Luma", "Chroma")
DUMP_SUFFIXES = ("_Partition.txt", "_Partition_FastOff_LFNST0.txt")


def build_parser():
    p = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    p.add_argument("--depthDir", required=True, help="directory of the Save_Depth_fal dumps")
    p.add_argument("--seqTable", required=True, help="sequence table (name,file,W,H,frames[,fps] per line)")
    p.add_argument("--outDir", required=True)
    p.add_argument("--qps", default="22,27,32,37")
    p.add_argument("--comps", default="Luma,Chroma")
    p.add_argument("--ssRatio", default=8, type=int, help="temporal sub-sampling of the dumped frames (CreateDataSet.py:292)")
    p.add_argument("--dataType", default="Train")
    p.add_argument("--chromaFactor", default="ref", choices=["ref", "1", "2"])
    p.add_argument("--keepInconsistent", action="store_true", help="exit 0 and write MSBT even where status bit 1 or 4 is set")
    p.add_argument("--device", default=0, type=int)
    return p


def find_dump(depth_dir, seq, qp, comp):
    for suf in DUMP_SUFFIXES:
        path = os.path.join(depth_dir, "%s_QP%d_%s%s" % (seq, qp, comp, suf))
        if os.path.isfile(path):
            return path
    return None


def plan(args, tool="gen_labels"):
    """Validates every flag and finds every dump -> (qps, comps, [(name, W, H, sub frames)], {(comp, qp, name): path}).
    SystemExit(2) on the first problem: nothing has touched the GPU yet.  Shared with label_partition (`tool`: the name in messages),
    whose arguments have no dataType."""
    def fail(msg):
        print(tool + ": " + msg, file=sys.stderr)
        raise SystemExit(2)
    try:
        qps = [int(q) for q in str(args.qps).split(",") if q.strip()]
    except ValueError:
        fail("--qps must be comma-separated integers, got %r" % args.qps)
    if not qps or any(q < 0 or q > 63 for q in qps):
        fail("--qps must name QPs in 0..63")
    comps = [c.strip() for c in str(args.comps).split(",") if c.strip()]
    if not comps or any(c not in COMPS for c in comps):
        fail("--comps must be a subset of Luma,Chroma, got %r" % args.comps)
    if args.ssRatio < 1:
        fail("--ssRatio must be >= 1")
    if hasattr(args, "dataType") and (not args.dataType or os.sep in args.dataType):
        fail("--dataType must be a plain name")
    if not os.path.isdir(args.depthDir):
        fail("--depthDir %s is not a directory" % args.depthDir)
    if not os.path.isfile(args.seqTable):
        fail("--seqTable %s not found" % args.seqTable)
    try:
        names, _, width, height, _, sub, _ = load_sequences_info(args.seqTable, args.ssRatio)
    except (ValueError, IndexError) as e:
        fail("--seqTable %s: %s" % (args.seqTable, e))
    if not names:
        fail("--seqTable %s lists no sequence" % args.seqTable)
    seqs = list(zip(names, width, height, sub))
    dumps, missing = {}, []
    for comp in comps:
        for qp in qps:
            for name, _, _, _ in seqs:
                path = find_dump(args.depthDir, name, qp, comp)
                if path is None:
                    missing.append("%s_QP%d_%s{%s}" % (name, qp, comp, ",".join(DUMP_SUFFIXES)))
                dumps[(comp, qp, name)] = path
    if missing:
        fail("missing dump(s) in %s: %s" % (args.depthDir, "; ".join(missing)))
    return qps, comps, seqs, dumps


def main(argv=None):
    args = build_parser().parse_args(argv)
    qps, comps, seqs, dumps = plan(args)
    os.makedirs(args.outDir, exist_ok=True)
    eng = None
    bad_pairs = 0
    for comp in comps:
        cf = 2 if (args.chromaFactor == "2" and comp == "Chroma") else 1
        for qp in qps:
            qs, bs, ds, unknown = [], [], [], 0
            for name, w, h, f in seqs:
                q, b, d, unk = E.output_block_partition_map(dumps[(comp, qp, name)], w, h, f, 64, comp == "Chroma", return_unknown=True)
                qs.append(q); bs.append(b); ds.append(d)
                unknown += unk
            qt, bt, dire = np.concatenate(qs), np.concatenate(bs), np.concatenate(ds)
            if eng is None:
                eng = E.Engine(args.device)
            msbt, st = eng.gen_seq_sub_map(qt - np.uint8(1), bt, dire, is_luma=(cf == 1), return_status=True)
            stem = os.path.join(args.outDir, "%s_%s_QP%d_" % (args.dataType, comp, qp))
            np.save(stem + "QTdepth_Block8.npy", qt)
            np.save(stem + "BTdepth_Block16.npy", bt)
            np.save(stem + "MSdirection_Block16.npy", dire)
            np.save(stem + "MSBTstatus.npy", st)
            counts = {bit: int(np.count_nonzero(st & bit)) for bit in (1, 2, 4)}
            refused = (counts[1] or counts[4]) and not args.keepInconsistent
            if not refused:
                np.save(stem + "MSBTdepth_Block16.npy", msbt)
            print("%s QP%d: %d blocks, cf %d, unknown split codes %d; status bit1 (inconsistent) %d, bit2 (qt > 3) %d, bit4 (leaf budget) %d"
                  % (comp, qp, len(qt), cf, unknown, counts[1], counts[2], counts[4]))
            print("Validate: %d" % int(np.sum(bt - msbt[:, 2, :, :])))      # GenMSBtMap.py:489, u8 arithmetic as there
            if refused:
                print("%s QP%d: MSBTdepth not written (--keepInconsistent writes it)" % (comp, qp), file=sys.stderr)
                bad_pairs += 1
    if eng is not None:
        eng.close()
    return 3 if bad_pairs else 0


if __name__ == "__main__":
    sys.exit(main())
