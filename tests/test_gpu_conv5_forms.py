"""The 5x5 Cout-64 convolutions in their three-workgroup forms (conv_f16x3.hip: conv_h2_kernel<5,5,4,0,1> and <5,5,4,2,0>), on the f16x3
datapath through pmp_debug_run_resblock, at the smallest shapes at which a form can go wrong: N = 2 blocks on maps of 16x16 (one tile, all
four borders), 32x32 (every tile a corner) and 48x32 (non-square, an interior column of tiles); RB(32,64,5) - the 32-channel LDS shortcut -
and RB(64,64,5) with its identity residual, each with and without the pool.

The yardstick is the convolution sweep's (tests/test_gpu_conv_sweep.py): every element of .t and of the output against the float64 bound
of oracle/layers64.py built from the kernels' own inputs, in poisoned workspaces; the launches are the ones the dispatch table
(oracle/conv_cases.py) predicts.  One case drives each launch's split-2 store to 1.02 and 0.97 of 65504: the range flag rises and stays
clear.  And the results are the bits of the two-workgroup kernels they replace: the .t and output tensors of RB(32,64,5) at 32x32, N = 2,
and the records of `bench.py --batch 8 --dump-outputs`, against tests/golden/conv5_forms.npz, which tools/gen_golden_conv5_forms.py took
from the library of the commit before the forms changed."""
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

import gpu_rig
from oracle import conv_cases as CC
from oracle import taps as T
from test_gpu_conv_sweep import check_case, out_ratio

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "conv5_forms.npz")
MAPS = ((16, 16), (32, 32), (48, 32))
RECORD_ARRAYS = ("hor", "ver", "qt", "dire")


def form_cases():
    rng = np.random.default_rng(20261020)
    out = []
    for h, w in MAPS:
        for cin in (32, 64):
            for pool in (False, True):
                out.append(CC._case(rng, "f16x3", len(out), n=2, h=h, w=w, cin=cin, cout=64, k=5, pool=pool))
    return out


CASES = form_cases()
IDENTITY_CASE = next(c for c in CASES if (c["h"], c["w"], c["cin"], c["pool"]) == (32, 32, 32, False))

eng = gpu_rig.engine_fixture(threads=16, setup=lambda e: T.taps_on(e, True), poison=2)


def bits_sha256(t):
    """sha256 of a tap's values as float32 bytes (the taps are float32 values held in float64: the conversion is exact)."""
    return hashlib.sha256(np.ascontiguousarray(t.numpy(), np.float32).tobytes()).hexdigest()


def identity_digests(e):
    """{"rb.t": sha256, "rb": sha256} of IDENTITY_CASE's two launches."""
    _, t_in, y, sat, kern, _ = check_case(e, IDENTITY_CASE, *CC.tensors(IDENTITY_CASE))
    assert not sat and kern == CC.expected_kernels(IDENTITY_CASE, fusion=False), (sat, kern)
    return {"rb.t": bits_sha256(t_in), "rb": bits_sha256(y)}


def bench_records(outdir, lib=None):
    """The records of one luma step of 8 blocks, as bench.py --dump-outputs writes them."""
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "1", "--warmup", "0", "--batch", "8", "--cpu-sample", "0",
           "--no-extras", "--dump-outputs", str(outdir)] + (["--lib", lib] if lib else [])
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    return {k: np.load(os.path.join(str(outdir), k + ".npy")) for k in RECORD_ARRAYS}


@pytest.mark.parametrize("c", CASES, ids=[c["id"] for c in CASES])
def test_form_against_float64(eng, c):
    rt, t_in, y, sat, kern, ins = check_case(eng, c, *CC.tensors(c))
    want = CC.expected_kernels(c, fusion=False)
    assert kern == want and want[0] == "conv_h2_kernel<5,5,4,0,1>", (kern, want)
    ry = out_ratio(c, t_in, y, ins)
    print("%s: max |gpu - ref64| / bound .t %.3f (%s), out %.3f (%s)" % (c["id"], rt, kern[0], ry, kern[1]))
    assert rt <= 1.0 and ry <= 1.0, (rt, ry)
    assert not sat, "range flag raised in range"


def test_range_flag_rises_at_each_store(eng):
    """Each launch's split-2 store driven to 1.02 and 0.97 of 65504 * 2^E, as the sweep does: raised, clear."""
    c = next(c for c in CASES if (c["h"], c["w"], c["cin"], c["pool"]) == (16, 16, 32, False))
    x, w0, w2, wsc, gate = CC.tensors(c)
    _, t_in, y, sat, kern, _ = check_case(eng, c, x, w0, w2, wsc, gate)
    assert not sat
    for i, tensor in ((0, t_in), (1, y)):
        E = c["exp_x"] if i == 0 else c["exp_out"]
        top = float(tensor.abs().max())
        got = []
        for f in (1.02, 0.97):
            s = np.float32(f * 65504.0 * 2.0 ** E / top)
            args = (x, w0 * s, w2 / s, wsc, gate) if i == 0 else (x, w0, w2 * s, wsc * s, gate)
            got.append(check_case(eng, c, *args)[3])
        print("%s: range flag %s at 1.02 / 0.97 of 65504 * 2^E" % (kern[i], got))
        assert got == [1, 0], (kern[i], got)


def test_resblock_bits_are_the_two_workgroup_kernels(eng):
    gold = np.load(GOLDEN)
    got = identity_digests(eng)
    for k, v in got.items():
        assert v == str(gold["sha256_" + k]), "%s of %s differs from the kernels before the change" % (k, IDENTITY_CASE["id"])


def test_bench_records_are_the_two_workgroup_kernels(tmp_path):
    gold = np.load(GOLDEN)
    got = bench_records(tmp_path / "out")
    for k in RECORD_ARRAYS:
        assert got[k].dtype == gold[k].dtype and got[k].shape == gold[k].shape, k
        assert got[k].tobytes() == gold[k].tobytes(), "%s differs from the library before the change" % k
