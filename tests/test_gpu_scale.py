"""GPU tests at the sizes and world sizes the driver's round-end runs use:
  * the logit TAIL at BASELINE.json configs[1]'s real size - 4096 fresh blocks, default datapath - against the torch oracle, for the two
    worst-conditioned nets (Luma QP22, QP27), with the fp32 MFMA datapath (the range guard's re-run) on the same blocks;
  * a dress rehearsal of several ranks on the ONE GPU of the test box (gloo carries the collectives): bench.py --gpus 4 and the driver
    --gpus 4 on a ragged geometry, files byte-identical to one rank;
  * RCCL itself on the hardware that is there: a one-rank "nccl" process group (device_id=) through parallel.preflight,
    parallel.gather_records on a CUDA tensor, parallel.all_reduce_sum, and bench.py's device-tensor gather on its side stream."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import conftest  # noqa: F401 - puts tools/ on sys.path
import trained_like  # tools/trained_like.py: test-weight data (round 6: out of the product package)

from oracle import parity as Y

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-3
# Ranks of the one-GPU rehearsals.  The test box is shared: at most six processes may hold its GPU at once, and the pytest process
# holds it too once an earlier test has made a GPU call.  Four ranks keep a margin and still shard rows unevenly (27 rows -> 7,7,7,6).
RANKS = 4


def _clean_env(**extra):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT", "MASTER_ADDR", "PMP_DIST_FORCE")}
    env.update(PYTHONPATH=ROOT, **extra)
    return env


# ------------------------------------------------------------------------------------------------ the tail at full size
@pytest.mark.parametrize("comp,qp,n,mtt", [("Luma", 22, 4096, "trained_like"), ("Luma", 27, 2048, "uniform"), ("Luma", 32, 1024, "uniform"),
                                           ("Luma", 37, 1024, "trained_like"), ("Chroma", 22, 4096, "uniform")])
def test_full_size_logit_tail_default_datapath_and_guard_fallback(comp, qp, n, mtt):
    """4096 fresh recipe-R luma blocks (the campaign's seeds, tests/campaign_gpu.py): max |logit - oracle| < 1e-3 on the default f16x3
    datapath and on the exact fp32 MFMA datapath the range guard falls back to.  The 512-block tests sit at 1.9e-4; the tail at this
    size is 6.2e-4 / 5.6e-4 (profiles/r03_parity_campaign.txt) - Luma_Q's conditioning at low QP, the torch oracle itself is 3.3e-4
    from fp64-accumulated convolutions on those blocks - so this is the test that notices a kernel change eating the margin.
    The MAXIMUM over 4096 blocks is one sample of a chaotic tail: every change of summation order in the first layers moved it (6.2e-4,
    6.7e-4, 7.9e-4 over the builds of round 4; 7.9e-4 ... 8.7e-4 at 15 840 blocks) while the distribution stayed where it was (p99
    1.9e-4, p99.9 4.4-4.5e-4) and the HIP path stayed as close to fp64-accumulated convolutions as the oracle is
    (profiles/r04_campaign_config4_all.txt).  The tolerance is asserted on the maximum, the trip wire on the quantiles - for BOTH datapaths
    (round 5: the fp32 fallback is 7.6e-4 from the oracle on Luma QP27 at 15 840 blocks, profiles/r04_campaign_config4_all.txt; its old
    6.5e-4 bound on the maximum was a sample of the same chaotic tail).  Round 5 also puts Chroma QP22 at full size and Luma QP32 / QP37 at
    1024 blocks under the driver's eyes, and halves Luma QP27 to 2048 to pay for them (the oracle costs ~75 s per 4096 luma blocks on 16
    host threads and the suite has a time budget; every net at 4096 and 15 840 blocks: tests/campaign_gpu.py).
    Round 6: the Luma QP22 case at 4096 blocks and Luma QP37 run on the TRAINED-LIKE MTT weights (synth.py; the uniform
    synthetic ones keep Luma QP27 / QP32, Chroma QP22, bench.py's parity sample and test_config2_full_batch_properties) - the absolute 1e-3
    on every one of 4096 blocks of a net with trunks at 1e3 and gate products at 1e4, no re-run - and the split flags of those device
    logits are the oracle's, bit for bit.  The fp32 fallback keeps a bound on its maximum again (8.5e-4: 7.6e-4 is the largest value any
    campaign saw on it) beside the quantile trip wire."""
    from pmp_vvc_tip2023_amd import engine, synth
    y, u, v = synth.recipe_r_blocks(n, 5000 + qp + (0 if comp == "Luma" else 500))
    wbd = trained_like.msbd_weights(comp, qp) if mtt == "trained_like" else None      # None: the shipped or synthetic net, on both sides
    want = Y.oracle_logits(comp, qp, y, u, v, wbd)
    e = engine.Engine(0, allow_synthetic_mtt=True)
    try:
        out = {}
        e.load(comp, qp, msbd_weights=wbd)
        for prec in ("f16x3", "fp32"):
            e.set_precision(prec)
            hor, ver, q8, d8, qt, bt, dire = e.infer_postprocess(comp, qp, y, u, v, want_logits=True)
            assert not e.saturated() and e.saturation_reruns() == 0
            if prec == "f16x3":
                assert Y.flags_equal((hor, ver, q8, d8), Y.oracle_flags(comp, qt, bt, dire))
            out[prec] = per_block = Y.per_block_error((qt, bt, dire), want)
            print("\n  %s QP%d (%s MTT weights) %-5s %d blocks: max |logit - oracle| %.2e (margin %.2fx inside 1e-3), per block median %.1e p99 %.1e p99.9 %.1e"
                  % (comp, qp, mtt, prec, n, per_block.max(), TOL / per_block.max(), np.median(per_block), np.quantile(per_block, 0.99),
                     np.quantile(per_block, 0.999)), flush=True)
        for prec, pb in out.items():
            assert pb.max() < (TOL if prec == "f16x3" else 8.5e-4), "%s QP%d on %s: logits off by %g" % (comp, qp, prec, pb.max())
            q99, q999 = np.quantile(pb, 0.99), np.quantile(pb, 0.999)
            assert q99 < 2.5e-4 and q999 < 5.5e-4, "%s QP%d on %s: the tail moved: p99 %.2e, p99.9 %.2e (round 4, f16x3: 1.9e-4 / 4.4e-4 at Luma QP22)" % (comp, qp, prec, q99, q999)
    finally:
        e.close()


# ------------------------------------------------------------------------------------------------ several ranks, rehearsed on one GPU
def test_bench_world4_rehearsal():
    """`python bench.py --gpus 4` as its own launcher: four fresh rank processes share the box's GPU (gloo), one JSON line with
    n_gpus = 4, four times the blocks, and the multi_gpu diagnostics of all four ranks."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", str(RANKS), "--steps", "2", "--warmup", "1", "--batch", "16",
                        "--cpu-sample", "0", "--no-extras"], capture_output=True, text=True, timeout=1500, env=_clean_env(PMP_DIST_BACKEND="gloo"))
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, r.stdout
    d = json.loads(lines[0])
    assert d["n_gpus"] == RANKS and d["config"]["blocks_per_gpu"] == 16 and d["config"]["global_blocks"] == RANKS * 16 and d["scaling"] == "weak"
    m = d["multi_gpu"]
    assert d["rccl_ranks"] == RANKS and m["rccl_ranks"] == RANKS and m["backend"] == "gloo" and m["gather_bytes_per_step"] == RANKS * 16 * 1344
    assert len(m["ms_per_step_by_rank"]) == RANKS and all(t > 0 for t in m["ms_per_step_by_rank"]) and len(m["gather_ms_by_rank"]) == RANKS
    assert "preflight ok: %d ranks" % RANKS in r.stderr
    assert d["value"] > 0 and abs(d["value"] - RANKS * 16 / 4.0 / (d["ms_per_step"] * 1e-3)) < 0.01 * d["value"]
    # round 5: every rank's own clock / socket power (sysfs hwmon, sampled by a host thread during the timed region) and workspace, so that a
    # sub-linear multi-GPU curve can be read from the JSON alone: node power (clocks below the 1-GPU line's), the exchange, or one slow rank
    for key in ("sclk_mhz_mean_by_rank", "sclk_mhz_min_by_rank", "power_w_mean_by_rank", "power_w_max_by_rank", "workspace_bytes_by_rank"):
        assert len(m[key]) == RANKS, key
    assert all(w > 0 for w in m["workspace_bytes_by_rank"])
    from pmp_vvc_tip2023_amd import sensors
    probe = sensors.read_once(sensors.for_torch_device(0))       # a box that hides the hwmon nodes reports nulls, by design: then only the shape is checked
    if probe["sclk_mhz"] is not None:
        assert all(c is not None and 100 < c < 3000 for c in m["sclk_mhz_mean_by_rank"]), m["sclk_mhz_mean_by_rank"]
        assert d["sensors"]["samples"] >= 1 and d["sensors"]["source"].startswith("sysfs hwmon")
    if probe["power_w"] is not None:
        assert all(p is not None and 50 < p < 2000 for p in m["power_w_mean_by_rank"]), m["power_w_mean_by_rank"]


def test_bench_under_torch_distributed_run():
    """The driver's own command for N > 1 - `python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1
    --master-port P bench.py --gpus N ...` - with N = 2 on the box's one GPU (gloo): the launcher's RANK / LOCAL_RANK / WORLD_SIZE /
    MASTER_* reach bench.py, rank 0 prints the one JSON line, nobody re-launches anything."""
    import socket
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
                        "--master-port", str(port), os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "1", "--batch", "16",
                        "--cpu-sample", "0", "--no-extras"], capture_output=True, text=True, timeout=900, env=_clean_env(PMP_DIST_BACKEND="gloo"))
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.strip().startswith("{")]
    assert len(lines) == 1, r.stdout
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["config"]["global_blocks"] == 32 and d["scaling"] == "weak" and d["multi_gpu"]["rccl_ranks"] == 2
    assert d["steps"] == 2 and d["warmup"] == 1 and d["value"] > 0
    assert "preflight ok: 2 ranks" in r.stderr


def test_driver_world4_rehearsal_ragged(tmp_path):
    """The driver with --gpus 4 on a geometry that does not divide: 9 sub-sampled frames of 5 x 3 blocks = 27 block rows over 4 ranks
    (three ranks take 7 rows, one takes 6; frames straddle ranks).  Sharded emission and --emit gather both write the bytes of one rank."""
    from pmp_vvc_tip2023_amd import inference_qbd as D, synth
    inp = tmp_path / "in"; cfg = tmp_path / "cfg"
    inp.mkdir(); cfg.mkdir()
    w, h, fr = 320, 192, 9
    with open(inp / "table.txt", "w") as f:
        f.write("SeqR,SeqR_320x192_30.yuv,%d,%d,%d,30\n#end!!!!\n" % (w, h, fr))
    y, u, v = synth.recipe_r_frames(fr, h, w, 191)
    with open(inp / "SeqR_320x192_30.yuv", "wb") as f:
        for i in range(fr):
            f.write(y[i].tobytes()); f.write(u[i].tobytes()); f.write(v[i].tobytes())
    with open(cfg / "SeqR.cfg", "w") as f:
        f.write("InputFile : SeqR_320x192_30.yuv\nInputBitDepth : 8\n")
    common = ["--inputDir", str(inp), "--seqTable", "table.txt", "--cfgDir", str(cfg), "--ssRatio", "1", "--seqNum", "1", "--qps", "22", "--allowSyntheticMTT"]
    D.main(["--jobID", "one", "--outDir", str(tmp_path / "o1")] + common)
    d1 = tmp_path / "o1" / "one" / "PartitionMat"
    names = sorted(os.listdir(d1))
    assert len(names) == 2
    for job, extra in (("w4", []), ("w4g", ["--emit", "gather"])):
        r = subprocess.run([sys.executable, "-m", "pmp_vvc_tip2023_amd.inference_qbd", "--jobID", job, "--outDir", str(tmp_path / job), "--gpus", str(RANKS)]
                           + extra + common, env=_clean_env(PMP_DIST_BACKEND="gloo"), cwd=ROOT, capture_output=True, text=True, timeout=1500)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
        assert "ranks: %d (gloo)" % RANKS in r.stdout                      # rank 0's progress lines arrive on the launcher's stdout
        dn = tmp_path / job / job / "PartitionMat"
        assert names == sorted(os.listdir(dn))
        for nme in names:
            assert open(d1 / nme, "rb").read() == open(dn / nme, "rb").read(), (job, nme)


# ------------------------------------------------------------------------------------------------ RCCL on the box that is there
_RCCL_ONE_RANK = r"""
import os, sys
import numpy as np
import torch
import torch.distributed as dist
from pmp_vvc_tip2023_amd import parallel
dev = torch.device("cuda", 0)
torch.cuda.set_device(dev)
rank, world, local = parallel.init_process_group(dev, force=True)
assert dist.is_initialized() and dist.get_backend() == "nccl" and dist.get_world_size() == 1
info = parallel.preflight(dev)                                   # gather + all_reduce of device tensors, contents verified
assert info["ranks"] == 1 and info["backend"] == "nccl", info
assert parallel.relax_timeout() == 1800.0
rec = torch.randint(0, 255, (37, 1344), dtype=torch.uint8, device=dev)
got = parallel.gather_records(rec, 37, dev)                      # the device-tensor branch: RCCL gather, one D2H on rank 0
assert isinstance(got, np.ndarray) and np.array_equal(got, rec.cpu().numpy())
got = parallel.gather_records(rec.cpu().numpy(), 37, dev)        # numpy in: staged to the device first
assert np.array_equal(got, rec.cpu().numpy())
tab = np.arange(24, dtype=np.int64).reshape(4, 6)
assert np.array_equal(parallel.all_reduce_sum(tab, dev), tab)    # the sharded emission's size table
dist.barrier()
torch.cuda.synchronize(dev)
dist.destroy_process_group()
print("RCCL one-rank ok: preflight %.1f ms" % info["ms"])
"""


def test_rccl_one_rank_process_group():
    """Nothing in the multi-GPU path had ever touched RCCL on hardware.  A one-rank "nccl" group on the test
    box's GPU loads librccl, creates the communicator with device_id= as parallel.init_process_group does for N ranks, and runs the
    device-tensor branches of preflight / gather_records / all_reduce_sum.  Fresh process: never a GPU-touched process re-executed."""
    r = subprocess.run([sys.executable, "-c", _RCCL_ONE_RANK], env=_clean_env(PMP_DIST_BACKEND="nccl", HSA_ENABLE_IPC_MODE_LEGACY="0"),
                       cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    assert "RCCL one-rank ok" in r.stdout


def test_bench_rccl_branch_one_rank():
    """bench.py with PMP_DIST_FORCE=1: the N > 1 step - records gathered as device tensors over RCCL on the bench's side stream,
    events around the collective - on a one-rank group.  The line says backend nccl, rccl_ranks 1."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "2", "--warmup", "1", "--batch", "64", "--cpu-sample", "0",
                        "--no-extras"], capture_output=True, text=True, timeout=900,
                       env=_clean_env(PMP_DIST_FORCE="1", PMP_DIST_BACKEND="nccl", HSA_ENABLE_IPC_MODE_LEGACY="0"))
    assert r.returncode == 0, r.stderr[-3000:]
    d = json.loads([l for l in r.stdout.splitlines() if l.strip()][0])
    m = d["multi_gpu"]
    assert d["n_gpus"] == 1 and m["backend"] == "nccl" and m["rccl_ranks"] == 1 and m["gather_bytes_per_step"] == 64 * 1344
    assert m["gather_ms"] > 0 and "preflight ok: 1 ranks over nccl" in r.stderr
