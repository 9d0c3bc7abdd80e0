"""Network inference + post-processing driver: drop-in for the reference's Inference_QBD.py.

    python -m pmp_vvc_tip2023_amd.inference_qbd --jobID 0000 --inputDir /input/ --outDir /output/ \\
           --batchSize 200 --startSeqID 0 --seqNum 22                     (Inference_QBD.py:257-267, same flags)
    torchrun --nproc-per-node 8 -m pmp_vvc_tip2023_amd.inference_qbd ...  (blocks sharded over the GPUs)

Output, byte-compatible with what the patched VTM-10.0 reads (EncAppCfg.cpp:4234-4404):
    <outDir>/<jobID>/PartitionMat/<seq-file-stem>_<Luma|Chroma>_QP<22|27|32|37>_PartitionMat.txt   (:153,:237)
    <outDir>/<jobID>/Time_Sta_<start>_<end>.txt    5 comma-terminated columns x 4 QP rows per sequence  (:243-253)

Mirrors, function by function: load_sequences_info (:48-76), import_yuv420 (:78-102), output_block_yuv (:104-149,
on the GPU), inference_VVC_seqs (:151-255).  Differences, all flags with the reference's values as defaults where
the reference hard-codes them:
  --seqTable   Training_Sequences.txt in the reference (:50, file not shipped); default VVC_Test_Sequences.txt
  --cfgDir     ".\\per-sequence" (:162)                      --modelDir "./CTU_Models" (:219-220), falls back to weights/
  --ssRatio    30 (:26); the codec demo uses TemporalSubsampleRatio 8 (encoder_intra_vtm.cfg:61)
  sequence file stem: the reference's rstrip(".yuv") strips a character SET (:166); a real suffix strip is used
  (identical for every name in VVC_Test_Sequences.txt and what EncAppCfg.cpp:4235-4242 expects).
  Nets are loaded once per (component, QP) instead of once per sequence (:208-224).
  --batchSize is the reference's blocks-per-pass knob; passes of 4096 blocks are used unless --strictBatch (identical results).
  Frames are uploaded once per sequence and cut on the GPU; the blocks stay device-resident for all passes (--hostBlocks
  restores the reference's host-side block arrays).
  Multi-GPU (--gpus N / torchrun): a sequence's BLOCK ROWS are sharded over the ranks; every rank formats and pwrites the text of
  its own rows (emit.py; the ranks exchange only a table of byte counts), so nothing funnels through rank 0.  --emit gather keeps
  the older path: RCCL gather of the 1344-byte records to rank 0, which writes the file alone.
  The job is pipelined: the next sequence's frames are read on a host thread while this one runs; while the GPU runs pass k+1
  the host copies pass k's records (pinned buffers), formats and writes them.
"""
import argparse
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor
from dataclasses import dataclass, field

import numpy as np

from . import emit
from . import engine as E
from . import parallel

QPS = (22, 27, 32, 37)
COMP_COLUMN = {"Luma": 0, "Chroma": 1}
DEFAULT_MODEL_DIR = "./CTU_Models"                 # Inference_QBD.py:219-220


def load_sequences_info(seqs_info_path, ss_ratio, num=None):
    """Inference_QBD.py:48-76: rows `name,file,W,H,frames,fps` until a line containing 'end!!!!'."""
    data = []
    with open(seqs_info_path, "r") as fp:
        for line in fp:
            if "end!!!!" in line:
                break
            line = line.rstrip("\n").strip()
            if line:
                data.append(line.split(","))
    if num is not None:
        data = data[:num]
    names = [d[0] for d in data]
    files = [d[1] for d in data]
    width = [int(d[2]) for d in data]
    height = [int(d[3]) for d in data]
    frames = [int(d[4]) for d in data]
    sub = [(f + ss_ratio - 1) // ss_ratio for f in frames]
    blocks = [(w // 64) * (h // 64) * s for w, h, s in zip(width, height, sub)]
    return names, files, width, height, frames, sub, blocks


def parse_seq_cfg(path):
    """Inference_QBD.py:171-186: InputFile and InputBitDepth from a VTM per-sequence cfg ('#' starts a comment)."""
    seq_path, is10bit = None, False
    with open(path) as fp:
        for line in fp:
            if "InputFile" in line:
                line = line.rstrip("\n").split("#")[0].replace(" ", "")
                seq_path = line.split(":", 1)[1]
            elif "InputBitDepth" in line:
                line = line.rstrip("\n").split("#")[0].replace(" ", "")
                is10bit = line.split(":", 1)[1] == "10"
    if seq_path is None:
        raise ValueError("%s: no InputFile entry" % path)
    return seq_path, is10bit


def import_yuv420(file_path, width, height, frm_num, SubSampleRatio=1, is10bit=False, frames=None, alloc=None):
    """Inference_QBD.py:78-102: every SubSampleRatio-th frame of a planar 4:2:0 file -> y[F,H,W], u,v[F,H/2,W/2].
    frames=(k0, k1) reads only the sub-sampled frames k0 <= k < k1 (a rank's shard: nothing else is touched on disk).
    alloc(shape, dtype) supplies the arrays (pinned host memory in the driver); the planes are read straight into them."""
    pix = width * height
    sub = (frm_num + SubSampleRatio - 1) // SubSampleRatio
    k0, k1 = (0, sub) if frames is None else (max(0, int(frames[0])), min(sub, int(frames[1])))
    nf = max(0, k1 - k0)
    dt = np.uint16 if is10bit else np.uint8
    alloc = alloc or np.zeros
    y = alloc((nf, height, width), dt); u = alloc((nf, height // 2, width // 2), dt); v = alloc((nf, height // 2, width // 2), dt)
    bps = 2 if is10bit else 1
    with open(file_path, "rb", buffering=0) as fp:
        for k in range(k0, k1):
            i = k * SubSampleRatio
            fp.seek(i * (pix * 3 // 2) * bps, 0)
            _read_plane(fp, y[k - k0]); _read_plane(fp, u[k - k0]); _read_plane(fp, v[k - k0])
    return y, u, v


def _read_plane(fp, a):
    """One plane straight into its (C-contiguous) array: no intermediate copy, whatever memory `a` lives in."""
    buf = memoryview(a.reshape(-1)).cast("B")
    got = 0
    while got < len(buf):
        k = fp.readinto(buf[got:])
        if not k:
            raise IOError("%s: short read (the file holds fewer frames than the sequence table says)" % getattr(fp, "name", "input"))
        got += k


def shard_frames(lo, hi, per_frame):
    """Sub-sampled frames [f0, f1) that hold blocks lo <= b < hi (per_frame blocks each, frame-major order)."""
    return lo // per_frame, (hi + per_frame - 1) // per_frame


def strip_yuv_suffix(name):
    return name[:-4] if name.endswith(".yuv") else name


def build_parser():
    p = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    p.add_argument("--jobID", type=str, default="0000")
    p.add_argument("--inputDir", type=str, default="/input/")
    p.add_argument("--outDir", type=str, default="/output/")
    p.add_argument("--batchSize", default=200, type=int, help="blocks per forward pass (library chunk)")
    p.add_argument("--startSeqID", default=0, type=int)
    p.add_argument("--seqNum", default=22, type=int)
    # paths the reference hard-codes
    p.add_argument("--seqTable", default="VVC_Test_Sequences.txt")
    p.add_argument("--cfgDir", default=os.path.join(".", "per-sequence"))
    p.add_argument("--modelDir", default=DEFAULT_MODEL_DIR)
    p.add_argument("--ssRatio", default=30, type=int, help="temporal sub-sampling (Inference_QBD.py:26)")
    p.add_argument("--qps", default="22,27,32,37")
    p.add_argument("--comps", default="Luma,Chroma")
    p.add_argument("--device", default=None, type=int, help="GPU index (default: LOCAL_RANK)")
    p.add_argument("--gpus", default=1, type=int,
                   help="shard every sequence's blocks over this many GPUs of the node: started without a launcher the driver spawns "
                        "its own rank processes (one per GPU, RCCL gather of the records to rank 0); under torchrun it is one rank")
    p.add_argument("--binary", action="store_true", help="also write <name>_PartitionMat.pmpb (binary side channel, include/pmp.h)")
    p.add_argument("--strictBatch", action="store_true",
                   help="run exactly --batchSize blocks per pass (default: the library's 4096-block chunk; same results)")
    p.add_argument("--allowSyntheticMTT", action="store_true",
                   help="run the MTT nets on the documented SYNTHETIC weights when a <Comp>_BD_<qp> model file is missing (the "
                        "reference checkout ships none); without this flag a missing model file is an error, as in the reference")
    p.add_argument("--precision", default="f16x3", choices=["f16x3", "bf16x6", "fp32"],
                   help="convolution datapath (all fp32-equivalent, include/pmp.h): f16x3 is fastest and range-guarded")
    p.add_argument("--emit", default="sharded", choices=["sharded", "gather"],
                   help="sharded (default): every rank formats and pwrites the text of its own block rows, the ranks exchange only byte "
                        "counts; gather: RCCL gather of the records to rank 0, which writes the file alone")
    p.add_argument("--emitThreads", default=0, type=int, help="formatter / writer threads per rank (0 = cores / ranks, at most 8)")
    p.add_argument("--overlap", action="store_true",
                   help="turn the library's overlap mode on (include/pmp.h: pmp_set_overlap): a pass of >= 1024 blocks runs as two chunks on "
                        "two streams, so one chunk's small launches fill the gaps of the other's large ones; bit-identical files.  Opt-in "
                        "(round 6): it takes 0.2-1.7 %% off a bare 4096-block step but nothing off a whole job (8 x 4K frames, all eight "
                        "files: 1.702 s on, 1.701 s off, profiles/r05e_driver_bench.txt) and costs a second workspace")
    p.add_argument("--m2p", default=None, metavar="SPEC",
                   help="Map2Partition thresholds for both components, e.g. 'lamb1=0.6,thd=0.45' (keys lamb1..lamb5, thd; the rest keep "
                        "the reference's 0.7,0.7,1.5,0.3,0.7 | 0.5; domain in include/pmp.h: pmp_partition_params)")
    p.add_argument("--m2pChroma", default=None, metavar="SPEC",
                   help="the same for chroma only, applied on top of --m2p")
    p.add_argument("--hostBlocks", action="store_true",
                   help="keep the cut blocks in host memory and upload them for every (component, QP) pass, as the reference "
                        "does; default: frames are uploaded once, cut on the GPU and the blocks stay device-resident")
    return p


class PinnedPool:
    """Page-locked host buffers, reused: frames go up (and records come down) by DMA without a staging copy, and pinning - a
    system call per buffer - is paid once per size, not once per sequence.  torch is the allocator here, nothing else."""

    def __init__(self, torch):
        import threading
        self.torch, self.free, self.lock = torch, [], threading.Lock()   # the reader thread takes, the main thread gives

    def take(self, nbytes):
        nbytes = max(int(nbytes), 1)
        with self.lock:
            best = None
            for i, t in enumerate(self.free):
                if t.numel() >= nbytes and (best is None or t.numel() < self.free[best].numel()):
                    best = i
            if best is not None:
                return self.free.pop(best)
        return self.torch.empty(nbytes, dtype=self.torch.uint8, pin_memory=True)

    def give(self, t):
        with self.lock:
            if len(self.free) >= 8:                   # bound the pinned footprint: drop the smallest
                self.free.sort(key=lambda x: x.numel())
                self.free.pop(0)
            self.free.append(t)

    def array(self, shape, dtype):
        """(ndarray view of a pinned buffer, the buffer) - give() the buffer back when the array is dead."""
        n = int(np.prod(shape)) * np.dtype(dtype).itemsize
        t = self.take(n)
        return t.numpy()[:n].view(dtype).reshape(shape), t


class DeviceBlocks:
    """Device-resident blocks of one sequence shard: the sub-sampled frames are uploaded once, cut by
    pmp_cut_blocks_device (Inference_QBD.py:104-149 on the GPU) and reused by all eight (component, QP) passes; only the split
    flags (1344 B per block) come back.  torch is the device allocator here, nothing else."""
    lookahead = True     # enqueue() returns while the GPU works: run_sequence loads the nets of the pass after next beside it

    def __init__(self, eng, dev, y, u, v, bitdepth, lo, hi):
        import torch
        self.eng, self.torch, self.dev = eng, torch, dev
        F, H, W = y.shape
        per_frame = (H // 64) * (W // 64)

        def up(a):   # torch has no uint16: 10-bit planes travel as int16 bit patterns
            return torch.from_numpy(np.ascontiguousarray(a).view(np.int16) if a.dtype == np.uint16 else np.ascontiguousarray(a)).to(dev, non_blocking=True)
        ty, tu, tv = up(y), up(u), up(v)
        self.by = torch.empty((F * per_frame, 68, 68), dtype=torch.uint8, device=dev)
        self.bu = torch.empty((F * per_frame, 34, 34), dtype=torch.uint8, device=dev)
        self.bv = torch.empty((F * per_frame, 34, 34), dtype=torch.uint8, device=dev)
        torch.cuda.synchronize(dev)
        eng.cut_blocks_device(ty.data_ptr(), tu.data_ptr(), tv.data_ptr(), F, H, W, bitdepth, self.by.data_ptr(), self.bu.data_ptr(), self.bv.data_ptr())
        eng.synchronize()
        del ty, tu, tv
        self.by, self.bu, self.bv = self.by[lo:hi], self.bu[lo:hi], self.bv[lo:hi]   # leading-dimension slices: still contiguous
        self.n = hi - lo

    def enqueue(self, comp, qp):
        """Enqueue one pass on the library's stream and return at once: the shard's packed records u8[n, 1344] as a DEVICE tensor
        (a fresh one per pass - the previous pass's records may still be on their way to the host).  They are final after
        eng.synchronize() (include/pmp.h: the range guard is settled there)."""
        chroma = comp == "Chroma"
        rec = self.torch.empty((self.n, parallel.RECORD), dtype=self.torch.uint8, device=self.dev)
        self.eng.infer_postprocess_records_device(comp, qp, self.by.data_ptr(), self.bu.data_ptr() if chroma else None,
                                                  self.bv.data_ptr() if chroma else None, self.n, rec.data_ptr())
        return rec

    def collect(self, rec):
        """The pass behind `rec` is done and final (range guard settled): the engine has been synchronised, here is the tensor."""
        self.eng.synchronize()
        return rec

    def infer_postprocess_records(self, comp, qp):
        """One pass, finished: the records as a device tensor."""
        return self.collect(self.enqueue(comp, qp))


class HostBlocks:
    """The same interface over blocks in HOST arrays (--hostBlocks, or torch without a GPU): every pass uploads them again, as the
    reference does, and runs inside collect() - which also loads that pass's nets.  Without blocks - a rank without rows, a
    sequence without a full 64x64 block - collect() gives u8[0, 1344] and makes no GPU call."""
    lookahead = False

    def __init__(self, job, blocks=None):
        self.job, self.blocks, self.n = job, blocks, (blocks[0].shape[0] if blocks else 0)

    def enqueue(self, comp, qp):
        return comp, qp

    def collect(self, handle):
        self.job.load_weights(*handle)
        if not self.n:
            return np.zeros((0, parallel.RECORD), np.uint8)
        return parallel.pack_records(*self.job.eng.infer_postprocess(*handle, *self.blocks))


def open_blocks(job, seq):
    """The block source of this rank's shard of `seq`: by default the frames go up once, are cut on the GPU and the blocks never
    leave it."""
    if seq.planes is None:
        return HostBlocks(job)
    bitdepth, o = 10 if seq.is10bit else 8, seq.f0 * seq.per_frame
    if job.torch_dev is not None:
        return DeviceBlocks(job.eng, job.torch_dev, *seq.planes, bitdepth, seq.lo - o, seq.hi - o)
    return HostBlocks(job, [a[seq.lo - o:seq.hi - o] for a in job.eng.output_block_yuv(*seq.planes, bitdepth)])


def _emit(rec, save_path, frames, height, width, binary):
    h, v, q, d = parallel.unpack_records(rec)
    E.write_partition_file(save_path, frames, height, width, h, v, q, d)
    if binary:
        E.write_partition_binary(save_path[:-4] + ".pmpb", frames, height, width, h, v, q, d)


def resolve_model_dir(model_dir):
    """--modelDir as given must exist; only the untouched default (./CTU_Models, Inference_QBD.py:219-220) falls back to
    the packaged weights/ directory when it is absent.  A mistyped directory is an error, not a silent fallback."""
    if os.path.isdir(model_dir):
        return model_dir
    if model_dir == DEFAULT_MODEL_DIR:
        return None                                   # weights.default_weight_dir()
    raise FileNotFoundError("--modelDir %s does not exist" % model_dir)


def _resolve(path, base):
    return path if os.path.isabs(path) or os.path.exists(path) else os.path.join(base, path)


class Stages:
    """Wall-clock seconds the MAIN thread of this rank spent per stage (tools/driver_bench.py prints them)."""
    NAMES = ("setup", "weights", "read_wait", "h2d_cut", "first_enqueue", "gpu_wait", "enqueue", "d2h", "emit_start", "emit_finish", "gather", "drain", "teardown")

    def __init__(self):
        self.t = dict.fromkeys(self.NAMES, 0.0)
        self.prefetch_read = 0.0        # seconds the reader thread spent in file I/O (hidden behind the passes unless read_wait shows it)
        self.blocks = 0
        self.passes = 0

    def add(self, name, t0):
        t1 = time.perf_counter()
        self.t[name] += t1 - t0
        return t1


LAST_STAGES = None      # the Stages of the last inference_VVC_seqs() run in this process (tools/driver_bench.py reads it)


def partition_params(args):
    """--m2p / --m2pChroma -> {comp: thresholds} through the library's own parser (pmp_parse_partition_params); a bad spec is an
    error before any GPU work."""
    luma = E.parse_partition_params(args.m2p or "")
    chroma = E.parse_partition_params(args.m2pChroma or "", luma)
    return {"Luma": luma, "Chroma": chroma}


class Job:
    """What one rank's process holds for the whole job: its place among the ranks, the engine, the devices, the pinned pool - and,
    once inference_VVC_seqs has made them, the reader and the sink, so that release() can reach them."""
    reader = sink = None

    def __init__(self, rank, world, eng, device=None, torch_dev=None, pinned=None):
        self.rank, self.world, self.eng, self.device, self.torch_dev, self.pinned = rank, world, eng, device, torch_dev, pinned
        self.announced = set()

    def load_weights(self, comp, qp):
        """Weights once per (comp, qp), not once per sequence; rank 0 says where each net came from the first time it sees it."""
        self.eng.load(comp, qp)
        if self.rank == 0:
            for (net, q), src in sorted(self.eng.provenance.items()):
                if (net, q) not in self.announced:
                    self.announced.add((net, q))
                    print("weights %s QP%d: %s" % (net, q, src), flush=True)
                    if str(src).startswith("synthetic") and "warned" not in self.announced:
                        self.announced.add("warned")
                        print("WARNING: MTT nets run on SYNTHETIC weights (--allowSyntheticMTT): the PartitionMat files are not usable "
                              "for encoding", file=sys.stderr, flush=True)

    def close(self):
        """The normal end, at the same point on every rank."""
        self.eng.close()
        if self.world > 1:
            import torch.distributed as dist
            dist.barrier()
            dist.destroy_process_group()

    def release(self):
        """After a failure: give up what THIS process owns and nothing else.  No drain, finish, barrier or any other collective -
        the other ranks may be gone, and parallel.spawn_ranks ends the job on the first failing rank anyway."""
        if self.reader is not None:
            self.reader.close(wait=False)
        if self.sink is not None:
            self.sink.abandon()
        self.eng.close()


def open_job(args):
    """Rank and device, the engine with its settings, the rendezvous with its preflight collective, torch's device, the pinned pool."""
    rank, world, local = parallel.env_world()
    if world > 1 and args.device is not None:
        raise SystemExit("--device selects the GPU of a single-process run; with %d ranks every rank takes the GPU of its LOCAL_RANK" % world)
    dev_id = args.device if args.device is not None else local
    backend = os.environ.get("PMP_DIST_BACKEND", "nccl")
    if world > 1:
        import torch
        ndev = torch.cuda.device_count()
        if local >= ndev:
            if backend == "nccl":   # two RCCL ranks on one device fail or hang at init (duplicate GPU): refuse with a readable message
                raise SystemExit("rank %d of %d has no GPU of its own (%d visible): RCCL needs one GPU per rank (PMP_DIST_BACKEND=gloo "
                                 "lets several ranks share a GPU, for smoke tests only)" % (rank, world, ndev))
            dev_id = local % max(ndev, 1)
    model_dir = resolve_model_dir(args.modelDir)
    try:
        m2p = partition_params(args)
    except E._lib.PmpError as e:
        raise SystemExit("--m2p / --m2pChroma: %s" % e)
    eng = E.Engine(dev_id, weight_dir=model_dir, allow_synthetic_mtt=args.allowSyntheticMTT)
    for comp, prm in m2p.items():            # every rank: each one post-processes its own shard
        eng.set_partition_params(comp, **prm)
        if rank == 0 and prm != E.DEFAULT_PARTITION_PARAMS:
            print("Map2Partition thresholds (%s): %s" % (comp, ", ".join("%s=%.9g" % kv for kv in prm.items())), file=sys.stderr, flush=True)
    # --batchSize is the reference's blocks-per-forward-pass (a GPU memory knob there).  Results do not depend on it (tested:
    # ragged chunks are bit-identical to one pass); small passes only leave most of an MI355X idle, so it is ignored unless
    # --strictBatch asks for it (clamped to the library's 4096-block pass; the reference accepts any value)
    eng.set_chunk(min(max(1, args.batchSize), 4096) if args.strictBatch else 4096)
    eng.set_precision(args.precision)
    eng.set_overlap(args.overlap)            # opt-in: measured to buy nothing at job level (see --overlap)
    try:
        return Job(rank, world, eng, *_open_devices(args, rank, world, dev_id))
    except BaseException:
        eng.close()
        raise


def _open_devices(args, rank, world, dev_id):
    """(the collectives' device after rendezvous and preflight, torch's device for the blocks, the pinned pool); None where unused."""
    device = None
    if world > 1:
        import torch
        device = torch.device("cuda", dev_id)
        torch.cuda.set_device(device)
    parallel.init_process_group(device)
    if world > 1:
        info = parallel.preflight(device)            # a broken RCCL / IPC setup fails HERE, with a message, not in the first real pass
        parallel.relax_timeout()                     # PMP_DIST_TIMEOUT_S bounded the rendezvous; the passes' collectives get PMP_DIST_COLLECTIVE_TIMEOUT_S
        if rank == 0:
            print("ranks: %d (%s), first collective %.1f ms" % (info["ranks"], info["backend"], info["ms"]), flush=True)
    if args.hostBlocks:
        return device, None, None
    try:
        import torch
    except ImportError:
        return device, None, None
    if not torch.cuda.is_available():
        print("WARNING: torch sees no GPU although the library runs on one: blocks stay on the HOST (as with --hostBlocks)",
              file=sys.stderr, flush=True)
        return device, None, None
    return device, torch.device("cuda", dev_id), PinnedPool(torch)


@dataclass
class Sequence:
    """One sequence as the reader hands it to the passes: its geometry, this rank's shard of its blocks and - where the shard has
    any - the frames that hold them."""
    name: str
    stem: str                   # of the output files' names
    width: int
    height: int
    sub_numfrm: int
    is10bit: bool
    per_frame: int              # blocks per frame, n_total in the whole sequence
    n_total: int
    lo: int                     # this rank's blocks [lo, hi) ...
    hi: int
    g_lo: int                   # ... which sharded emission takes as whole block rows [g_lo, g_hi) (emit.py)
    g_hi: int
    f0: int = 0                 # the first sub-sampled frame in `planes`
    planes: tuple = None        # (y, u, v) of the frames that hold blocks lo..hi; None: the shard has no block, nothing was read
    bufs: list = field(default_factory=list)     # the pinned buffers behind the planes
    read_s: float = 0.0         # what the reader thread spent on it

    def give_back(self, pinned):
        """The blocks are cut: the frames go, their pinned buffers return to the pool."""
        for t in self.bufs:
            pinned.give(t)
        self.planes, self.bufs = None, []


class SequenceReader:
    """The reader: one thread, one sequence ahead of the passes.  A rank reads only the frames that hold its own block rows.
    Iterating yields the Sequences; the thread's I/O time goes to Stages.prefetch_read, the main thread's wait to read_wait."""

    def __init__(self, job, args, table, seq_ids, st):
        self.job, self.args, self.table, self.seq_ids, self.st = job, args, table, list(seq_ids), st
        self.pool = ThreadPoolExecutor(max_workers=1)
        self.nxt = self.pool.submit(self.load, self.seq_ids[0]) if self.seq_ids else None

    def load(self, seq_id):
        t0 = time.perf_counter()
        args, rank, world, pinned = self.args, self.job.rank, self.job.world, self.job.pinned
        names, files, widths, heights, frames, sub_frames, _ = self.table
        width, height, sub_numfrm = widths[seq_id], heights[seq_id], sub_frames[seq_id]
        seq_path, is10bit = parse_seq_cfg(os.path.join(args.cfgDir, names[seq_id] + ".cfg"))
        bh, bw = height // 64, width // 64
        per_frame = bh * bw
        if args.emit == "sharded":      # whole block rows per rank (emit.py)
            g_lo, g_hi = emit.shard_rows(sub_numfrm, bh, rank, world)
            lo, hi = g_lo * bw, g_hi * bw
        else:                           # contiguous block ranges, gathered to rank 0
            lo, hi = parallel.shard_bounds(per_frame * sub_numfrm, rank, world)
            g_lo = g_hi = 0
        seq = Sequence(names[seq_id], strip_yuv_suffix(files[seq_id]), width, height, sub_numfrm, is10bit, per_frame,
                       per_frame * sub_numfrm, lo, hi, g_lo, g_hi)
        if hi > lo and per_frame:
            seq.f0, f1 = shard_frames(lo, hi, per_frame)
            alloc = None
            if pinned is not None:
                def alloc(shape, dtype):
                    a, t = pinned.array(shape, dtype)
                    seq.bufs.append(t)
                    return a
            seq.planes = import_yuv420(_resolve(seq_path, args.inputDir), width, height, frames[seq_id], args.ssRatio, is10bit,
                                       frames=(seq.f0, f1), alloc=alloc)
        seq.read_s = time.perf_counter() - t0
        return seq

    def __iter__(self):
        for i in range(len(self.seq_ids)):
            tw = time.perf_counter()
            seq = self.nxt.result()
            self.nxt = self.pool.submit(self.load, self.seq_ids[i + 1]) if i + 1 < len(self.seq_ids) else None
            self.st.prefetch_read += seq.read_s
            self.st.add("read_wait", tw)
            yield seq

    def close(self, wait=True):
        self.pool.shutdown(wait=wait, cancel_futures=True)


class ShardedSink:
    """--emit sharded: every rank formats and pwrites its own block rows (emit.ShardEmitter, owned here).  Device records come down
    into a pinned double buffer, slot k & 1 for pass k, and the emitter reads a slot until finish() of its pass has returned.  The
    rule that keeps that safe is this class's alone: put(k) copies into its slot FIRST - the slot's last user, pass k-2, was
    finished by put(k-1) - then finishes pass k-1, whose formatting ran beside pass k on the GPU, then starts pass k.
    The collectives, at the same points on every rank: finish() (the size all-reduce) once per pass, in put() of the next pass or
    in end_sequence(); drain() (a barrier) once per sequence in end_sequence() and once in close()."""

    def __init__(self, emitter, pinned, st, binary=False):
        self.emitter, self.pinned, self.st, self.binary = emitter, pinned, st, binary
        self.slots, self.busy, self.prev = [None, None], [False, False], None      # prev: (the emitter's pending pass, its slot)

    def put(self, k, save_path, seq, records):
        tw, s, n = time.perf_counter(), k & 1, records.shape[0]
        assert not self.busy[s], "pinned record slot %d is still being formatted: finish() of its pass has not run" % s
        if isinstance(records, np.ndarray):
            host = np.ascontiguousarray(records).reshape(n, parallel.RECORD)
        else:                                       # D2H into a pinned buffer on torch's stream, next to pass k+1 on the library's
            need = n * parallel.RECORD
            if self.slots[s] is None or self.slots[s].numel() < need:
                self.slots[s] = self.pinned.take(need)
            ht = self.slots[s][:need].view(n, parallel.RECORD)
            ht.copy_(records)
            host = ht.numpy()
        tw = self.st.add("d2h", tw)
        tw = self._finish_prev(tw)                  # exchange the byte counts of pass k-1, queue its writes
        self.prev = self.emitter.start(save_path, seq.sub_numfrm, seq.height, seq.width, seq.g_lo, seq.g_hi, host, binary=self.binary), s
        self.busy[s] = True
        self.st.add("emit_start", tw)

    def _finish_prev(self, tw):
        if self.prev is None:
            return tw
        p, s = self.prev
        self.emitter.finish(p)
        self.busy[s], self.prev = False, None
        return self.st.add("emit_finish", tw)

    def end_sequence(self):
        tw = self._finish_prev(time.perf_counter())
        self.emitter.drain()                        # bound memory: a sequence's files are on disk before the next one starts
        self.st.add("drain", tw)

    def close(self):
        self.emitter.close()

    def abandon(self):
        self.emitter.pool.shutdown(wait=False, cancel_futures=True)


class GatherSink:
    """--emit gather: one gather of the records to rank 0 per pass (a collective: every rank's put() takes part), and rank 0 writes
    the file alone.  Text emission (645 k lines per 1080p frame and file) runs on writer threads - the C writer releases the GIL -
    so it overlaps the next (component, QP) pass instead of serialising rank 0."""

    def __init__(self, rank, device, st, binary=False):
        self.device, self.st, self.binary = device, st, binary
        self.writers, self.pending = (ThreadPoolExecutor(max_workers=4) if rank == 0 else None), []

    def put(self, k, save_path, seq, records):
        tw = time.perf_counter()
        rec = parallel.gather_records(records, seq.n_total, self.device)
        self.st.add("gather", tw)
        if self.writers:
            self.pending.append(self.writers.submit(_emit, rec, save_path, seq.sub_numfrm, seq.height, seq.width, self.binary))

    def end_sequence(self):
        tw = time.perf_counter()
        for fut in self.pending:
            fut.result()
        self.pending = []
        self.st.add("drain", tw)

    def close(self):
        if self.writers:
            self.writers.shutdown(wait=True)

    def abandon(self):
        if self.writers:
            self.writers.shutdown(wait=False, cancel_futures=True)


class TimeSta:
    """The Time_Sta log, Inference_QBD.py:243-253: per sequence four QP rows of block-loading, net Luma, net Chroma, post Luma and
    post Chroma seconds (the net column is inference + GPU post-processing here)."""

    def __init__(self, nseq):
        self.nseq = nseq
        self.block, self.net, self.post = np.zeros(max(nseq, 1)), np.zeros((max(nseq, 1), 4, 2)), np.zeros((max(nseq, 1), 4, 2))

    @staticmethod
    def cell(comp, qp):
        """(QP row, component column): Luma is column 0 whatever --comps lists; a QP outside the reference's four shares row 0."""
        return ((qp - 22) // 5 if qp in QPS else 0), COMP_COLUMN[comp]

    def total(self):
        return np.sum(self.block) + np.sum(self.net) + np.sum(self.post)

    def write(self, path):
        with open(path, "w") as fp:
            for si in range(self.nseq):
                for qi in range(4):
                    for s in (self.block[si], self.net[si, qi, 0], self.net[si, qi, 1], self.post[si, qi, 0], self.post[si, qi, 1]):
                        fp.write(str(s))
                        fp.write(",")
                    fp.write("\n")


def run_sequence(job, si, seq, src, sink, passes, save_dir, sta, st):
    """The pipeline schedule of one sequence and nothing else: pass k+1 is enqueued before the host touches pass k's records, the
    nets of pass k+2 are loaded beside it, the range guard of pass k is settled by collect(k).  Only the first pass's nets are
    loaded ahead of the GPU: the others go up while it runs the pass before theirs (30 ms of packing each, hidden)."""
    tw = time.perf_counter()
    if passes:
        job.load_weights(*passes[0])
    tw = st.add("weights", tw)
    cur = src.enqueue(*passes[0]) if passes else None
    tw = st.add("first_enqueue", tw)     # the job's first pass also sizes and allocates the activation workspace
    if len(passes) > 1:
        job.load_weights(*passes[1])     # next to pass 0 on the GPU
        st.add("weights", tw)
    for k, (comp, qp) in enumerate(passes):
        cell = (si,) + TimeSta.cell(comp, qp)
        save_path = os.path.join(save_dir, "%s_%s_QP%d_PartitionMat.txt" % (seq.stem, comp, qp))
        t0 = tw = time.perf_counter()
        reruns = job.eng.saturation_reruns()
        records = src.collect(cur)
        tw = st.add("gpu_wait", tw)
        if k + 1 < len(passes):          # the GPU starts on pass k+1 before the host touches pass k's records
            cur = src.enqueue(*passes[k + 1])
            tw = st.add("enqueue", tw)
            if k + 2 < len(passes) and src.lookahead:
                job.load_weights(*passes[k + 2])      # no-op after the first sequence
                st.add("weights", tw)
        sta.net[cell] = time.perf_counter() - t0
        if job.eng.saturation_reruns() != reruns:     # f16x3 range guard (include/pmp.h): results are right, the pass cost 3x
            print("WARNING: rank %d: %s %s QP%d drove an activation beyond the fp16 range of the f16x3 datapath; the pass was "
                  "re-run on the fp32 datapath (consider --precision bf16x6 for this model)" % (job.rank, seq.name, comp, qp), file=sys.stderr, flush=True)
        t0 = time.perf_counter()
        if job.rank == 0:
            print("Save:", save_path, flush=True)
        sink.put(k, save_path, seq, records)
        sta.post[cell] = time.perf_counter() - t0
    sink.end_sequence()


def inference_VVC_seqs(args):
    """Inference_QBD.py:151-255: the outline of a job.  A failure anywhere in it releases what this process owns (Job.release) and
    goes on up; the success path ends with the reader, the sink, the Time_Sta log and Job.close(), in that order."""
    global LAST_STAGES
    t_entry = time.perf_counter()
    job = open_job(args)
    try:
        save_dir = os.path.join(args.outDir, args.jobID, "PartitionMat")
        os.makedirs(save_dir, exist_ok=True)             # every rank writes its own rows into the files
        qps = [int(q) for q in args.qps.split(",") if q]
        passes = [(comp, qp) for comp in args.comps.split(",") if comp for qp in qps]
        table = load_sequences_info(_resolve(args.seqTable, args.inputDir), args.ssRatio)
        seq_ids = range(args.startSeqID, min(args.startSeqID + args.seqNum, len(table[0])))
        sta = TimeSta(len(seq_ids))
        st = LAST_STAGES = Stages()
        if args.emit == "sharded":
            job.sink = ShardedSink(emit.ShardEmitter(job.rank, job.world, threads=args.emitThreads, device=job.device), job.pinned, st, args.binary)
        else:
            job.sink = GatherSink(job.rank, job.device, st, args.binary)
        for comp, qp in passes:                          # a missing model file raises HERE, before any output
            job.eng.check_available(comp, qp)
        job.reader = SequenceReader(job, args, table, seq_ids, st)
        st.add("setup", t_entry)                         # context, rendezvous, the first read under way: once per job
        t0 = time.perf_counter()
        for si, seq in enumerate(job.reader):
            tw = time.perf_counter()
            if job.rank == 0:
                print(seq.name, flush=True)
            src = open_blocks(job, seq)
            seq.give_back(job.pinned)
            st.add("h2d_cut", tw)
            st.blocks += (seq.hi - seq.lo) * len(passes)
            st.passes += len(passes)
            sta.block[si] = time.perf_counter() - t0
            run_sequence(job, si, seq, src, job.sink, passes, save_dir, sta, st)
            del src                                      # the device blocks go before the next sequence's come
            t0 = time.perf_counter()
        tw = time.perf_counter()
        job.reader.close()
        job.sink.close()
        if job.rank == 0:
            sta.write(os.path.join(args.outDir, args.jobID, "Time_Sta_%d_%d.txt" % (args.startSeqID, args.startSeqID + args.seqNum)))
            print("Sum time:", sta.total())
        job.close()
        st.add("teardown", tw)
    except BaseException:
        job.release()
        raise
    return st


def launch_ranks(n, argv):
    """`--gpus N` without a launcher: N fresh rank processes (the parent makes no GPU call), all of them watched: the first rank
    that fails ends the job with its exit code (parallel.spawn_ranks)."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    rc, _ = parallel.spawn_ranks([sys.executable, "-m", "pmp_vvc_tip2023_amd.inference_qbd"] + list(argv), n,
                                 env_extra={"PYTHONPATH": root + os.pathsep + os.environ.get("PYTHONPATH", "")})
    return rc


def main(argv=None):
    argv = sys.argv[1:] if argv is None else list(argv)
    args = build_parser().parse_args(argv)
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        rc = launch_ranks(args.gpus, argv)
        if rc:
            raise SystemExit(rc)
        return
    t0 = time.time()
    inference_VVC_seqs(args)
    print("Total inference time:", time.time() - t0)


if __name__ == "__main__":
    main()
