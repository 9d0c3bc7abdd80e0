"""Validate a pair of nets against VTM labels on the GPU: Metrics.validation_QBD / pre_validation of the reference.

    python -m pmp_vvc_tip2023_amd.validate --dataDir D --modelDir M --comp Luma|Chroma --qp Q [--dataType Validate]
           [--mode qbd|bd|q|labels] [--batchSize 200] [--precision f16x3|bf16x6|fp32] [--perBlock out.npy] [--confusion] [--device 0]

Reads the reference's file names from --dataDir (Metrics.Load_Pre_VP_Dataset, Metrics.py:64-146):
    <dataType>_Y_Block68.npy                           u8[n,68,68]   (+ <dataType>_U_Block34.npy, _V_Block34.npy u8[n,34,34] for Chroma)
    <dataType>_<comp>_QP<qp>_QTdepth_Block8.npy        u8[n,8,8]     raw qtDepth
    <dataType>_<comp>_QP<qp>_MSBTdepth_Block16.npy     u8[n,3,16,16] (modes qbd, bd)
    <dataType>_<comp>_QP<qp>_MSdirection_Block16.npy   i8[n,3,16,16] (modes qbd, bd)
the three label files being what `python -m pmp_vvc_tip2023_amd.gen_labels` writes.  --mode qbd (default) is validation_QBD (both nets,
the QT net feeding the MTT net), bd is pre_validation predID 1 (the MTT net teacher-forced with the QT labels), q is predID 0 (the QT
net alone: only the <comp>_Q_<qp> model file is asked for).  Batches of --batchSize blocks in file order; the reference shuffles, so its numbers are defined up to the batch cut.
Prints ONE JSON object: the reference's numbers by name (q_L1, b0_L1 .., q_accu .., val_loss) plus comp, qp, mode, blocks, batches,
batch_size, precision and saturation_reruns.  --perBlock writes the per-block statistics float64[n,20] (include/pmp.h: pmp_val_stats).
--confusion adds "confusion": per map of the mode (q: qt; bd: bt0..2, dire0..2; qbd: all seven) the joint histogram of (label class,
predicted class) with what it says - label frequencies, hit / under / over for the depth maps, hit / missed / false / flipped for the
direction maps (validation.confusion_summary; include/pmp.h: pmp_val_confusion).  --mode labels is the census of a set's labels alone: the
same object with every prediction counted as "other", so that the label frequencies are what matters.  It reads the QTdepth file and, if
both are there, the MSBTdepth and MSdirection files; it needs no block file and no model file and runs no net.
Flags, files, dtypes and shapes are checked before anything touches the GPU: exit status 2 on the first problem.
"""
import argparse
import json
import os
import sys

import numpy as np

from . import validation as V
from .validation import NAMES             # the one table, also under the name the CLI's users know (validate.NAMES)

COMPS = ("Luma", "Chroma")


def build_parser():
    p = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    p.add_argument("--dataDir", required=True, help="directory of the block and label .npy files")
    p.add_argument("--modelDir", default=None, help="directory of the nets' weight files (default: the package's search path)")
    p.add_argument("--comp", required=True)
    p.add_argument("--qp", required=True, type=int)
    p.add_argument("--dataType", default="Validate")
    p.add_argument("--mode", default="qbd")
    p.add_argument("--batchSize", default=200, type=int)
    p.add_argument("--precision", default="f16x3")
    p.add_argument("--perBlock", default=None, help="write the per-block statistics float64[n,20] to this .npy file")
    p.add_argument("--confusion", action="store_true", help="add the confusion counts per map and their summary to the JSON object")
    p.add_argument("--allowSyntheticMtt", action="store_true", help="fall back to the synthetic MTT weights when the *_BD_* file is missing (tests)")
    p.add_argument("--device", default=0, type=int)
    return p


def plan(args):
    """Validates every flag and opens every file (memory-mapped) -> {"blocks": y or (y, u, v), "qt8", "msbt", "msdire", "n"}.
    SystemExit(2) on the first problem: nothing has touched the GPU yet."""
    def fail(msg):
        print("validate: " + msg, file=sys.stderr)
        raise SystemExit(2)
    if args.comp not in COMPS:
        fail("--comp must be Luma or Chroma, got %r" % args.comp)
    if args.mode not in V.MODES + ("labels",):
        fail("--mode must be qbd, bd, q or labels, got %r" % args.mode)
    if not 22 <= args.qp <= 41:
        fail("--qp must be in 22..41 (the rows of the reference's weight_mat), got %d" % args.qp)
    if args.batchSize < 1:
        fail("--batchSize must be >= 1")
    if args.precision not in ("f16x3", "bf16x6", "fp32"):
        fail("--precision must be f16x3, bf16x6 or fp32, got %r" % args.precision)
    if not args.dataType or os.sep in args.dataType:
        fail("--dataType must be a plain name")
    if not os.path.isdir(args.dataDir):
        fail("--dataDir %s is not a directory" % args.dataDir)
    if args.modelDir is not None and not os.path.isdir(args.modelDir):
        fail("--modelDir %s is not a directory" % args.modelDir)
    if args.perBlock is not None and not os.path.isdir(os.path.dirname(os.path.abspath(args.perBlock))):
        fail("--perBlock: directory of %s does not exist" % args.perBlock)

    if args.mode == "labels":
        if args.perBlock is not None:
            fail("--perBlock goes with the modes that run a net")
        stem = os.path.join(args.dataDir, "%s_%s_QP%d_" % (args.dataType, args.comp, args.qp))
        both = all(os.path.isfile(stem + tail) for tail in ("MSBTdepth_Block16.npy", "MSdirection_Block16.npy"))
        return V.read_set(args.dataDir, args.dataType, args.comp, args.qp, both, fail, with_blocks=False)
    return V.read_set(args.dataDir, args.dataType, args.comp, args.qp, args.mode != "q", fail)


def confusion_object(conf, mode):
    """The "confusion" entry of the JSON object: the summary of the maps that `mode` predicts"""
    summary = V.confusion_summary(conf)
    return {V.CONF_MAPS[i]: summary[V.CONF_MAPS[i]] for i in V.MODE_MAPS[mode]}


def main(argv=None):
    args = build_parser().parse_args(argv)
    d = plan(args)
    from . import engine as E
    eng = E.Engine(args.device, weight_dir=args.modelDir, allow_synthetic_mtt=args.allowSyntheticMtt)
    if args.mode == "labels":
        try:
            conf = eng.val_confusion(qt8=d["qt8"], msbt=d["msbt"], msdire=d["msdire"])
        finally:
            eng.close()
        print(json.dumps({"comp": args.comp, "qp": args.qp, "mode": "labels", "data_type": args.dataType, "blocks": d["n"],
                          "confusion": confusion_object(conf, "q" if d["msbt"] is None else "qbd")}))
        return 0
    try:
        eng.set_precision(args.precision)
        run = V.run(eng, args.mode, args.comp, args.qp, d["blocks"], d["qt8"], d["msbt"], d["msdire"], args.batchSize,
                    want_blocks=args.perBlock is not None, want_confusion=args.confusion)
        reruns = eng.saturation_reruns()
    finally:
        eng.close()
    if args.perBlock is not None:
        np.save(args.perBlock, run.block_stats)
    out = {"comp": args.comp, "qp": args.qp, "mode": args.mode, "data_type": args.dataType, "blocks": d["n"],
           "batches": (d["n"] + args.batchSize - 1) // args.batchSize, "batch_size": args.batchSize, "precision": args.precision,
           "saturation_reruns": reruns}
    out.update(zip(NAMES[args.mode], run.numbers()))
    if args.confusion:
        out["confusion"] = confusion_object(run.confusion(), args.mode)
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
