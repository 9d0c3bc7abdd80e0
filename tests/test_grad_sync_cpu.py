"""CPU: what data-parallel training (grad_sync.py, train_qbd --gpus N) stands on before it touches a GPU.

The bucket layout of pmp_grad_bucket_floats against a numpy restatement (tensor i at the sum of the earlier counts, each rounded up to a
multiple of 4) on the counts (1, 3, 4, 5, 1023), on a table of 97 tensors and on the bad tables; a rank's rows as a pure function of
(n, batchSize, world) on the issue's five cases, against the micro-batches of the one-rank run they must equal; train_qbd.plan's
refusals of --microBatch 0 and 257, of --gpus 3 --batchSize 1000 and of --device with several ranks, exit status 2, with no rank
started; `make traincheck` with the gradient buckets in its matrix; and the build's flags: nothing that lets the compiler reassociate
the chain of float32 additions of pmp_grad_sum_device.  The input condition of test_gpu_grad_bucket.py's order test is checked here too."""
import os
import re
import subprocess

import numpy as np
import pytest

import train_qbd_cases as TC
from conftest import ROOT
from pmp_vvc_tip2023_amd import grad_sync as G, train_qbd as T

import grad_bucket_cases as B

CSRC = os.path.join(ROOT, "pmp_vvc_tip2023_amd", "csrc")


@pytest.mark.parametrize("counts", [B.COUNTS, B.MANY, (1,), (4,), ((1 << 30) - 1, 7)])
def test_bucket_layout_equals_the_numpy_restatement(counts):
    from pmp_vvc_tip2023_amd import engine
    total, offsets = engine.grad_bucket_floats(counts)
    want_total, want_off = B.layout(counts)
    assert total == want_total and offsets == want_off
    assert total % 4 == 0 and all(o % 4 == 0 for o in offsets) and offsets[0] == 0
    assert all(b - a >= c for a, b, c in zip(offsets, offsets[1:] + [total], counts)), "the slices hold their tensors and do not overlap"


def test_bucket_layout_of_the_issues_counts():
    from pmp_vvc_tip2023_amd import engine
    assert engine.grad_bucket_floats((1, 3, 4, 5, 1023)) == (1044, [0, 4, 8, 12, 20])
    assert len(B.MANY) == 97


def test_bad_tables_are_refused():
    import ctypes as C
    from pmp_vvc_tip2023_amd import _lib, engine
    lib = _lib.load()
    arr = lambda v: (C.c_int64 * len(v))(*v)
    assert lib.pmp_grad_bucket_floats(0, arr([1]), None) == -1 and lib.pmp_grad_bucket_floats(-1, arr([1]), None) == -1
    assert lib.pmp_grad_bucket_floats(1, None, None) == -1
    for bad in (0, -1, 1 << 30, 1 << 40):
        assert lib.pmp_grad_bucket_floats(3, arr([5, bad, 7]), None) == -1, bad
        with pytest.raises(ValueError):
            engine.grad_bucket_floats([5, bad, 7])
    with pytest.raises(ValueError):
        engine.grad_bucket_floats([])
    assert lib.pmp_grad_bucket_floats(2, arr([5, 7]), None) == 16, "the offsets are optional"


SLICES = {(5, 5, 2): [(0, 3), (3, 5)], (2, 5, 2): [(0, 2), (2, 2)], (5, 5, 3): [(0, 2), (2, 4), (4, 5)],
          (200, 200, 8): [(25 * r, 25 * r + 25) for r in range(8)], (300, 400, 2): [(0, 200), (200, 300)]}


@pytest.mark.parametrize("case", list(SLICES))
def test_a_ranks_rows_are_the_micro_batches_of_the_one_rank_run(case):
    n, batch, world = case
    got = [G.rank_rows(n, batch, r, world) for r in range(world)]
    assert got == SLICES[case]
    m = G.rank_share(batch, world)
    micro = [(s, min(s + m, n)) for s in range(0, n, m)]                # Trainer.accumulate's cuts with --microBatch m
    active = G.active_ranks(n, batch, world)
    assert [got[r] for r in active] == micro and active == list(range(len(micro))) and 0 in active
    assert all(lo == hi for r, (lo, hi) in enumerate(got) if r not in active)
    assert sum(hi - lo for lo, hi in got) == n


def test_rank_rows_refuses_what_is_no_batch():
    for bad in [(6, 5, 0, 2), (5, 5, 2, 2), (5, 5, -1, 2), (5, 5, 0, 0), (-1, 5, 0, 2), (5, 0, 0, 2)]:
        with pytest.raises(ValueError):
            G.rank_rows(*bad)


@pytest.fixture(scope="module")
def data(tmp_path_factory):
    d = tmp_path_factory.mktemp("sets")
    TC.write_sets(str(d), "Luma", 22, n=3)
    return d


@pytest.mark.parametrize("flags,needle", [
    (dict(microBatch=0), "--microBatch"), (dict(microBatch=257), "--microBatch"), (dict(gpus=3, batchSize=1000), "--microBatch"),
    (dict(gpus=2, device=0), "--device"), (dict(gpus=2, device=1), "--device"), (dict(gpus=0), "--gpus"), (dict(gpus=65), "--gpus"),
    (dict(gpus=2, batchSize=5, microBatch=2), "--microBatch"),
])
def test_plan_refuses_the_new_flags_with_status_2(data, tmp_path, capsys, monkeypatch, flags, needle):
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    started = []
    monkeypatch.setattr(T, "launch_ranks", lambda *a: started.append(a) or 0)
    with pytest.raises(SystemExit) as e:
        T.main(TC.argv(data, tmp_path, "Luma", 0, **flags))
    assert e.value.code == 2 and not started
    err = capsys.readouterr().err
    assert err.startswith("train_qbd: ") and needle in err, err
    assert not os.path.exists(str(tmp_path / "0000")), "nothing was written"


def test_plan_takes_the_world_from_torchruns_environment(data, tmp_path, capsys, monkeypatch):
    argv = TC.argv(data, tmp_path, "Luma", 0, batchSize=600)
    args = T.build_parser().parse_args(argv)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    T.plan(args)                                                        # one rank: 600 runs as micro-batches
    assert args.gpus == 1 and args.microBatch == 256 and args.device == 0 and not args.deviceGiven
    monkeypatch.setenv("WORLD_SIZE", "2"); monkeypatch.setenv("RANK", "1"); monkeypatch.setenv("LOCAL_RANK", "1")
    with pytest.raises(SystemExit) as e:
        T.plan(args)
    assert e.value.code == 2 and "300 blocks a rank" in capsys.readouterr().err
    monkeypatch.setenv("WORLD_SIZE", "3")
    T.plan(args)
    assert T.job_world(args) == (1, 3, 1)


def test_gpus_starts_that_many_ranks_of_the_same_command(data, tmp_path, monkeypatch):
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    started = []
    monkeypatch.setattr(T, "launch_ranks", lambda n, argv: started.append((n, list(argv))) or 7)
    argv = TC.argv(data, tmp_path, "Luma", 0, gpus=2, batchSize=5, microBatch=3)
    assert T.main(argv) == 7 and started == [(2, argv)], "the ranks' exit status is the command's"


@pytest.mark.parametrize("how,status", [("agree", 0), ("apart", 4)])
def test_two_gloo_ranks_gather_in_rank_order_and_a_desync_ends_the_job_with_status_4(how, status, capfd, monkeypatch):
    """Two rank processes on the CPU (tests/grad_sync_ranks.py): grad_sync's gathers, and train_qbd's desync check, which names the rank"""
    import sys
    from pmp_vvc_tip2023_amd import parallel
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "PMP_DIST_FORCE"):
        monkeypatch.delenv(k, raising=False)
    rc, _ = parallel.spawn_ranks([sys.executable, os.path.join(ROOT, "tests", "grad_sync_ranks.py"), how], 2,
                                 env_extra={"PMP_DIST_BACKEND": "gloo", "PMP_DIST_TIMEOUT_S": "60"})
    err = capfd.readouterr().err
    assert rc == status == T.EXIT_DESYNC * (how == "apart"), err[-2000:]
    assert ("the parameters of rank 1 differ from rank 0's" in err) == (how == "apart"), err[-2000:]


def test_train_check_passes_with_the_gradient_buckets_in_its_matrix():
    """train_check.h with a main of its own under AddressSanitizer and UBSan: a stand-alone CPU program, built and run once."""
    r = subprocess.run(["make", "-s", "-C", CSRC, "traincheck"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "train_check: ok" in r.stdout, (r.stdout + r.stderr)[-2000:]
    main = open(os.path.join(CSRC, "train_check_main.cpp")).read()
    assert "grad_pack_refused(" in main and "grad_sum_refused(" in main and "grad_bucket_floats(" in main
    api = open(os.path.join(CSRC, "api_train.cpp")).read()
    assert "grad_pack_refused(" in api and "grad_sum_refused(" in api, "the entry points refuse through the same functions"


def test_the_library_exports_the_calls_and_the_engine_binds_them():
    from pmp_vvc_tip2023_amd import _lib, engine
    lib = _lib.load()
    assert all(hasattr(lib, k) for k in ("pmp_grad_bucket_floats", "pmp_grad_pack_device", "pmp_grad_sum_device"))
    assert callable(engine.Engine.grad_pack_device) and callable(engine.Engine.grad_sum_device) and callable(engine.grad_bucket_floats)
    header = open(os.path.join(ROOT, "include", "pmp.h")).read()
    assert "#define PMP_GRAD_SUM_MAX %d" % _lib.PMP_GRAD_SUM_MAX in header


def test_no_build_flag_lets_the_compiler_reassociate_the_sum():
    """pmp_grad_sum_device's chain ((a + b) + c) + ... is written as such; only a fast-math flag would let the compiler reorder it."""
    mk = open(os.path.join(CSRC, "Makefile")).read()
    for flag in ("-ffast-math", "-Ofast", "-fassociative-math", "-funsafe-math-optimizations", "-freciprocal-math", "-ffp-model=fast",
                 "-fapprox-func", "-fno-signed-zeros", "-ffinite-math-only"):
        assert flag not in mk, flag
    assert re.search(r"^EXTRA_train_step = .*-ffp-contract=off", mk, re.M)


def test_the_order_cases_tell_one_order_from_the_reverse():
    """The condition on the inputs of the GPU test: for every nsrc > 1 the float32 sum in the given order and in the reverse order
    differ on at least one element (for nsrc 2 no order can matter: a + b is b + a; there the sums are equal)."""
    for nsrc in B.NSRC:
        src = B.sources(nsrc)
        fwd, rev = B.ordered_sum(src), B.ordered_sum(src[::-1])
        assert fwd.dtype == np.float32 and np.isfinite(fwd).all()
        differ = int((fwd.view(np.uint32) != rev.view(np.uint32)).sum())
        assert (differ > 0) == (nsrc > 2), (nsrc, differ)
