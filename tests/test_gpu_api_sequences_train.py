"""The C ABI's state space walked through the training, label and loss calls and through changes of stream WITH WORK IN FLIGHT
(tests/test_gpu_api_sequences.py is the same idea for inference alone).  Every call of a context works in memory the caller never sees -
the activation workspace, the scratch of the loss and statistics kernels, the staging and logit buffers - so the library alone can order
two calls that it was handed on two streams (include/pmp.h, pmp_set_stream).  These tests hand it such calls and nothing else.

Rules of every test here.
  - WARM-UP: each call runs once on the context and is settled before a window opens, so that the workspace and every scratch and staging
    buffer have their final size: nothing is allocated with work in flight, and no kernel takes an address from data.
  - Every tensor is uploaded and every output filled (NaN; 0xFF bytes for d_saved) before the first call, then ONE torch.cuda.synchronize().
    Inside a window nothing synchronises the device, and every call writes to buffers of its own.
  - THE WINDOW WAS OPEN: the first call runs on a torch stream handed over with set_stream, and once the later calls are enqueued the test
    asserts `not first_stream.query()` - a condition, not a measurement: a case too small to hold it fails.  Where the later call is one that
    waits on the host by contract (a host-pointer call, a call that settles a pending range-guard re-run), the stream is queried right
    BEFORE that call instead, and the test says so.
  - Results are read only after a bare eng.synchronize(): the header's promise that this makes every *_device call final.
  - YARDSTICK: every output equals, bit for bit, the same call on a fresh, idle context in default settings (each family's own test ties
    that run to float64); the exact integer cases are compared with their table's float64 restatement as well.
The directed pairs print their first call's GPU time, taken by events around it alone on an idle context (the long trunk call on the
shared idle one; pair 3's inference call on the context under test, idle then); the walk has no long call and prints none."""
import functools

import numpy as np
import pytest
import torch

import conftest  # noqa: F401 - puts tools/ on sys.path
import trained_like  # tools/trained_like.py: test-weight data

import head_cases as H
import msbt_cases as MS
import qtail_cases as Q
import resblock_cases as K
import stem_cases as S
import train_loss_cases as TL
import train_rig as R
import trunk_cases as T
import val_cases as V
from oracle.parity import range_stress_weights

pytestmark = pytest.mark.gpu

P, up, nan = R.P, R.up, R.nan
LONG_N = 48                                        # the long call: trunk_M1's chain on n blocks of 64x64 (d_saved: 12.6 MB per block)
LONG_SHAPE = (LONG_N, 64, 64, 32, [(64, 5)] + [(64, 3)] * 5, 1)
ORDER = ("qt", "bt", "dire", "qt8", "msbt", "msdire")


# ---- a call on buffers of its own -----------------------------------------------------------------------------------------------
class Job:
    """One call, or a forward with its backward, on buffers of its own.  enqueue(e) makes the engine calls and nothing else; tensors()
    are the device tensors they write; table(e) (exact cases) compares with the float64 restatement, after the read point."""

    def __init__(self, name, enqueue, tensors, table=None, keep=None):
        self.name, self.enqueue, self._tensors, self.table, self.keep = name, enqueue, tensors, table, keep

    def tensors(self):
        return {k: v for k, v in self._tensors.items() if v is not None}


def _bits(t):
    return t.contiguous().view({1: torch.uint8, 4: torch.int32, 8: torch.int64}[t.element_size()])


def differing(job, ref):
    """{tensor: how many elements differ from the reference run's, bit for bit}, the equal ones left out."""
    got, want = job.tensors(), ref.tensors()
    assert sorted(got) == sorted(want), (job.name, sorted(got), sorted(want))
    bad = {k: int((_bits(got[k]) != _bits(want[k])).sum()) for k in got}
    return {k: "%d of %d" % (v, got[k].numel()) for k, v in bad.items() if v}


@functools.lru_cache(maxsize=None)
def block_case(name):
    c = K.make_exact(name)
    want = {k: K.as_f32(v) for k, v in K.restate(c).items()}
    c["t"], c["out"] = want["t"], want["out"]
    return c, want


def block_job(name):
    c, want = block_case(name)
    d = R.BlockDev(c)
    return Job("resblock " + name, lambda e: (d.forward(e), d.backward(e)), d.o, lambda e: R.check_bits(name, d.results(e), want))


@functools.lru_cache(maxsize=None)
def trunk_case(name):
    if name == "long":
        return T.make_case(LONG_SHAPE, 4801, exact=False), None
    c = T.make_exact(name)
    return c, {k: K.as_f32(v) for k, v in T.flat(T.restate(c)).items()}


def chain_job(what, dev, want):
    t = dict(dev.outputs())
    table = None if want is None else lambda e: R.check_bits(what, dev.results(e), want)
    return Job(what, lambda e: (dev.forward(e), dev.backward(e)), t, table, keep=dev)


def trunk_job(e, name):
    c, want = trunk_case(name)
    return chain_job("trunk " + name, R.TrunkDev(e, c), want)


def trunk_forward_job(e, name):
    """pmp_trunk_forward_device alone: y and d_saved."""
    dev = R.TrunkDev(e, trunk_case(name)[0])
    return Job("trunk forward " + name, dev.forward, {"y": dev.y, "d_saved": dev.saved}, keep=dev)


@functools.lru_cache(maxsize=None)
def tail_case(name):
    c, r = Q.exact(name)
    return c, {k: K.as_f32(v) for k, v in r.items()}


def tail_job(e, name):
    c, want = tail_case(name)
    return chain_job("qtail " + name, R.TailDev(e, c), want)


def stem_job(name):
    c, want = S.exact(name)
    d = R.StemDev(c)
    return Job("stem " + name, lambda e: (d.forward(e), d.backward(e)), dict(d.outputs()), lambda e: R.check_bits_same_keys(name, d.results(e), want),
               keep=d)


def head_job(name):
    c, want = H.exact(name)
    d = R.HeadDev(c)

    def table(e):
        got = d.results(e)
        for k, v in want.items():
            if v is None:
                assert k not in got or np.isnan(got[k]).all(), (name, k, "written without being asked for")
            else:
                assert H.same_bits(got[k], v), (name, k)
    return Job("head " + name, lambda e: (d.forward(e), d.backward(e)), d.o, table, keep=d)


def gate_job(count):
    c = H.gate_case(count)
    want = H.gate_reference(c, True)
    d = {k: up(c[k]) for k in ("x", "a", "g_y", "g_acc")}
    o = {k: nan(count) for k in ("y", "g_x", "g_a")}

    def enqueue(e):
        e.gate_forward_device(count, P(d["x"]), P(d["a"]), P(o["y"]))
        e.gate_backward_device(count, P(d["x"]), P(d["a"]), P(d["g_y"]), P(d["g_acc"]), P(o["g_x"]), P(o["g_a"]))

    def table(e):
        for k, v in want.items():
            assert H.same_bits(R.num(o[k]), v), ("gate", count, k)
    return Job("gate %d" % count, enqueue, o, table, keep=d)


@functools.lru_cache(maxsize=None)
def loss_inputs(n):
    """train_loss_cases' luma30_n17 tiled to n blocks -> (the case, the six arrays)."""
    c = TL.make("luma30_n17")
    pick = np.arange(n) % c["n"]
    return c, {k: np.ascontiguousarray(c[k][pick]) for k in ORDER}


def loss_job(n):
    """pmp_train_loss_device with gradients: the block partials go through the context's d_trainpart."""
    c, kw = loss_inputs(n)
    d = {k: torch.from_numpy(kw[k]).cuda() for k in ORDER}
    out = torch.full((14,), -1.0, dtype=torch.float64, device="cuda")
    g = {k: nan(*d[k].shape) for k in ("qt", "bt", "dire")}

    def enqueue(e):
        e.train_loss_device(c["comp"], c["qp"], *[P(d[k]) for k in ORDER], n, out.data_ptr(), out.data_ptr() + 104, P(g["qt"]), P(g["bt"]),
                            P(g["dire"]), params=c["lam"])
    return Job("train_loss %d" % n, enqueue, dict({"g_" + k: v for k, v in g.items()}, terms_loss=out), keep=d)


@functools.lru_cache(maxsize=None)
def val_inputs(n):
    """val_cases' qp32 tiled to n blocks."""
    c = V.make("qp32")
    pick = np.arange(n) % c["n"]
    return c, {k: np.ascontiguousarray(c[k][pick]) for k in ORDER}


def val_job(n):
    """pmp_val_stats_device without d_block_stats: the block partials go through the context's d_valpart."""
    c, kw = val_inputs(n)
    d = {k: torch.from_numpy(kw[k]).cuda() for k in ORDER}
    out = torch.full((20,), -1.0, dtype=torch.float64, device="cuda")
    return Job("val_stats %d" % n, lambda e: e.val_stats_device(c["qp"], *[P(d[k]) for k in ORDER], n, out.data_ptr(), None), {"stats": out}, keep=d)


def settled():
    """Between preparing tensors through torch and the first engine call: the one device-wide synchronisation of a test."""
    torch.cuda.synchronize()


# ---- the idle context: references, and the first call's time -------------------------------------------------------------------------
@pytest.fixture(scope="module")
def idle():
    """The shared fresh context of the training, label and loss references: default settings, one call at a time."""
    from pmp_vvc_tip2023_amd import engine
    e = engine.Engine(0)
    yield e
    e.close()


def idle_run(e, job):
    """job alone on the idle context e (on a stream of torch's, so that events can time it) -> (job, GPU milliseconds)."""
    s = torch.cuda.Stream()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    settled()
    e.set_stream(s.cuda_stream)
    try:
        a.record(s)
        job.enqueue(e)
        b.record(s)
        e.synchronize()
    finally:
        e.set_stream(0)
    b.synchronize()
    return job, a.elapsed_time(b)


_REF = {}


def reference(e, key, make):
    """The idle run of make(), once per key; left unchanged."""
    if key not in _REF:
        idle_run(e, make())                      # the context's own warm-up: the timed run allocates nothing
        _REF[key] = idle_run(e, make())
    return _REF[key]


def long_reference(idle):
    job, ms = reference(idle, "long", lambda: trunk_job(idle, "long"))
    print("the long call (trunk forward + backward, n = %d) alone on the idle context: %.2f ms" % (LONG_N, ms))
    return job


SHORT = {
    "resblock identity": lambda e: block_job("identity"),
    "resblock sc_5x5": lambda e: block_job("sc_5x5"),
    "trunk b_like": lambda e: trunk_job(e, "b_like"),
    "stem q_luma_one": lambda e: stem_job("q_luma_one"),
    "head b1_16x24": lambda e: head_job("b1_16x24"),
    "gate 1023": lambda e: gate_job(1023),
    "qtail nets": lambda e: tail_job(e, "nets"),
}


def short_reference(idle, key):
    return reference(idle, key, lambda: SHORT[key](idle))[0]


def _luma_weights(kind):
    from pmp_vvc_tip2023_amd import synth
    if kind == "benign":
        return synth.synth_msbd_weights("Luma", 22)
    if kind == "trained":
        return trained_like.msbd_weights("Luma", 22)
    return range_stress_weights()                              # "stress"


@functools.lru_cache(maxsize=None)
def block_pool():
    from conftest import golden
    from pmp_vvc_tip2023_amd import synth
    y, _, _ = synth.recipe_r_blocks(400, 99)
    y[:16] = golden("g1_qt.npz")["block_y"]
    return y


_INFER = {}


def infer_reference(kind, prec, scales=True):
    """Logits and records of the whole block pool on a fresh context in default settings with these weights on this datapath (scales:
    its calibrated f16x3 activation scales, as on the context under test; without them the range-stress weights fire the guard) -> dict
    of device tensors; once per (weights, datapath, scales)."""
    from pmp_vvc_tip2023_amd import engine
    if (kind, prec, scales) not in _INFER:
        y = block_pool()
        n = y.shape[0]
        e = engine.Engine(0, allow_synthetic_mtt=True)
        try:
            e.set_precision(prec)
            e.set_activation_scales(scales)
            e.load("Luma", 22, msbd_weights=_luma_weights(kind))
            d = torch.from_numpy(y).cuda()
            o = {"qt": nan(n, 64), "bt": nan(n, 768), "dire": nan(n, 768), "rec": torch.zeros((n, 1344), dtype=torch.uint8, device="cuda")}
            settled()
            e.infer_device("Luma", 22, d.data_ptr(), None, None, n, P(o["qt"]), P(o["bt"]), P(o["dire"]))
            e.infer_postprocess_records_device("Luma", 22, d.data_ptr(), None, None, n, P(o["rec"]))
            e.synchronize()
            _INFER[(kind, prec, scales)] = o
        finally:
            e.close()
    return _INFER[(kind, prec, scales)]


class Sliced(Job):
    """A reference that is rows [lo, lo + n) of infer_reference's tensors."""

    def __init__(self, ref, keys, lo, n):
        Job.__init__(self, "idle", None, {k: ref[k][lo:lo + n] for k in keys})


def infer_job(lo, n, records=False):
    """pmp_infer_device (logits into the caller's tensors) or pmp_infer_postprocess_records_device of blocks [lo, lo + n) of the pool."""
    d = torch.from_numpy(block_pool()[lo:lo + n]).cuda()
    if records:
        o = {"rec": torch.zeros((n, 1344), dtype=torch.uint8, device="cuda")}
        return Job("records %d" % n, lambda e: e.infer_postprocess_records_device("Luma", 22, d.data_ptr(), None, None, n, P(o["rec"])), o, keep=d)
    o = {"qt": nan(n, 64), "bt": nan(n, 768), "dire": nan(n, 768)}
    return Job("infer %d" % n, lambda e: e.infer_device("Luma", 22, d.data_ptr(), None, None, n, P(o["qt"]), P(o["bt"]), P(o["dire"])), o, keep=d)


# ---- the context under test ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def eng():
    """The context the windows open on: Luma QP22 loaded, everything else as created."""
    from pmp_vvc_tip2023_amd import engine
    e = engine.Engine(0, allow_synthetic_mtt=True)
    e.load("Luma", 22, msbd_weights=_luma_weights("benign"))
    yield e
    e.close()


@pytest.fixture(scope="module")
def streams():
    """s1 and three second streams, the same ones for the whole module."""
    return [torch.cuda.Stream() for _ in range(4)]


def warm(e, jobs):
    """Every call of a test once on the context, settled: buffers have their final size before the first window opens."""
    settled()
    for j in jobs:
        j.enqueue(e)
    e.synchronize()
    settled()


def check(e, pairs):
    """pairs = [(job, its idle reference)], after the bare eng.synchronize(): bits against the idle run, then the exact tables."""
    bad = {j.name: differing(j, ref) for j, ref in pairs}
    bad = {k: v for k, v in bad.items() if v}
    assert not bad, "differs from the idle context's run, bit for bit, in (call: tensor: elements): %s" % bad
    for j, _ in pairs:
        if j.table:
            j.table(e)


# ---- (a) directed pairs ------------------------------------------------------------------------------------------------------------
# 1. the long call on s1, then the short training calls on a second stream
@pytest.mark.parametrize("second", [1, 2, 3])
def test_training_calls_on_a_second_stream_while_a_trunk_runs_on_the_first(eng, idle, streams, second):
    s1, s2 = streams[0], streams[second]
    refs = [long_reference(idle)] + [short_reference(idle, k) for k in SHORT]
    warm(eng, [trunk_job(eng, "long")] + [SHORT[k](eng) for k in SHORT])
    jobs = [trunk_job(eng, "long")] + [SHORT[k](eng) for k in SHORT]
    settled()
    try:
        eng.set_stream(s1.cuda_stream)
        jobs[0].enqueue(eng)
        eng.set_stream(s2.cuda_stream)
        for j in jobs[1:]:
            j.enqueue(eng)
        assert not s1.query(), "the long call had finished before the short ones were enqueued: the case is too small"
        eng.synchronize()
    finally:
        eng.set_stream(0)
    check(eng, list(zip(jobs, refs)))


# 2. the trainer validates: the long call on s1, then a host-pointer inference on the context's own stream
def test_host_inference_on_the_own_stream_while_a_trunk_runs(eng, idle, streams):
    s1 = streams[0]
    y = block_pool()[20:26]
    want = infer_reference("benign", "f16x3")["rec"][20:26].cpu().numpy()
    ref = long_reference(idle)
    warm(eng, [trunk_job(eng, "long")])
    eng.infer_postprocess("Luma", 22, y)
    job = trunk_job(eng, "long")
    settled()
    try:
        eng.set_stream(s1.cuda_stream)
        job.enqueue(eng)
        eng.set_stream(0)
        # a host-pointer call returns final results, so it waits on the host: the window is shown open right before it
        assert not s1.query(), "the long call had finished before the host call was made: the case is too small"
        hor, ver, q8, d8 = eng.infer_postprocess("Luma", 22, y)
        eng.synchronize()
    finally:
        eng.set_stream(0)
    got = np.concatenate([hor.reshape(6, -1), ver.reshape(6, -1), q8.reshape(6, -1), d8.reshape(6, -1).view(np.uint8)], axis=1)
    assert np.array_equal(got, want), "the host call's records differ from the idle context's in %d bytes" % int((got != want).sum())
    check(eng, [(job, ref)])


# 3. an inference call that leaves nothing pending (fp32; f16x3 under PMP_SAT_IGNORE) on s1, then a ResidualBlock on s2
@pytest.mark.parametrize("prec,policy", [("fp32", "rerun"), ("f16x3", "ignore")])
def test_resblock_on_a_second_stream_while_an_unguarded_inference_runs(eng, idle, streams, prec, policy):
    s1, s2 = streams[0], streams[1]
    refs = [Sliced(infer_reference("benign", prec), ("qt", "bt", "dire"), 50, 300), short_reference(idle, "resblock sc_5x5")]
    try:
        eng.set_precision(prec)
        eng.set_saturation_policy(policy)
        warm(eng, [infer_job(50, 300), block_job("sc_5x5")])
        print("inference of 300 blocks on %s alone on the idle context: %.2f ms" % (prec, idle_run(eng, infer_job(50, 300))[1]))
        jobs = [infer_job(50, 300), block_job("sc_5x5")]
        settled()
        eng.set_stream(s1.cuda_stream)
        jobs[0].enqueue(eng)
        eng.set_stream(s2.cuda_stream)
        jobs[1].enqueue(eng)
        assert not s1.query(), "the inference call had finished before the ResidualBlock was enqueued: the case is too small"
        eng.synchronize()
    finally:
        eng.set_stream(0)
        eng.set_saturation_policy("rerun")
        eng.set_precision("f16x3")
    check(eng, list(zip(jobs, refs)))


# 4. a range-guard re-run is pending when a training call arrives: admit() settles first
def test_training_call_behind_a_pending_range_guard_rerun(eng, idle, streams):
    s1 = streams[0]
    refs = [long_reference(idle), Sliced(infer_reference("stress", "f16x3", scales=False), ("rec",), 100, 130), short_reference(idle, "trunk b_like")]
    try:
        eng.set_activation_scales(False)         # with the calibrated scales these weights stay inside the fp16 range
        eng.load("Luma", 22, msbd_weights=_luma_weights("stress"))
        warm(eng, [trunk_job(eng, "long"), infer_job(100, 130, records=True), trunk_job(eng, "b_like")])
        jobs = [trunk_job(eng, "long"), infer_job(100, 130, records=True), trunk_job(eng, "b_like")]
        settled()
        before = eng.saturation_reruns()
        eng.set_stream(s1.cuda_stream)
        jobs[0].enqueue(eng)                     # holds s1 busy, so that the inference call is certainly still in flight below
        jobs[1].enqueue(eng)
        assert eng.saturation_reruns() == before, "the re-run is still to come"
        # the training call settles what is pending, so it waits on the host: the window is shown open right before it
        assert not s1.query(), "the stream had drained before the training call was made: the case is too small"
        jobs[2].enqueue(eng)
        assert eng.saturation_reruns() > before, "the training call did not settle the pending re-run before it ran"
        eng.synchronize()
    finally:
        eng.set_stream(0)
        eng.set_activation_scales(True)
        eng.load("Luma", 22, msbd_weights=_luma_weights("benign"))
    check(eng, list(zip(jobs, refs)))


# 5. two calls that share a scratch buffer of the context (d_trainpart, d_valpart) on two streams.  "behind_trunk": the issue's 4096
# blocks, which take microseconds, queued behind the long trunk on s1 so that they are certainly not done when the second call is
# enqueued.  "alone": 32768 blocks (0.45 GB through the kernel) and nothing in front, so that the first call itself is still running:
# the two calls' block kernels and reductions can then meet in the scratch buffer.
BIG_N = 32768


@pytest.mark.parametrize("second", [1, 2, 3])       # as in pair 1: two streams that share a hardware queue serialise there by themselves
@pytest.mark.parametrize("front", ["behind_trunk", "alone"])
@pytest.mark.parametrize("family", ["train_loss", "val_stats"])
def test_two_calls_sharing_a_scratch_buffer_on_two_streams(eng, idle, streams, family, front, second):
    s1, s2 = streams[0], streams[second]
    make = loss_job if family == "train_loss" else val_job
    n1 = 4096 if front == "behind_trunk" else BIG_N
    first = [lambda e: trunk_job(e, "long")] if front == "behind_trunk" else []
    makers = first + [lambda e: make(n1), lambda e: make(5)]
    refs = ([long_reference(idle)] if first else []) + [reference(idle, (family, n), lambda: make(n)) for n in (n1, 5)]
    print("%s of %d blocks alone on the idle context: %.3f ms" % (family, n1, refs[-2][1]))
    refs = refs[:-2] + [refs[-2][0], refs[-1][0]]
    warm(eng, [m(eng) for m in makers])
    jobs = [m(eng) for m in makers]
    settled()
    try:
        eng.set_stream(s1.cuda_stream)
        for j in jobs[:-1]:
            j.enqueue(eng)
        eng.set_stream(s2.cuda_stream)
        jobs[-1].enqueue(eng)
        assert not s1.query(), "the first stream had drained before the second call was enqueued: the case is too small"
        eng.synchronize()
    finally:
        eng.set_stream(0)
    check(eng, list(zip(jobs, refs)))


# 7. the last call before the change of stream is one that DRAINS the stream in its middle: a re-run is pending on s1, the long trunk
# forward on s1 settles it (a host wait) and only then enqueues its own kernels, and the stream changes right behind it.  That work is
# in flight although the context had just been synchronised: the short calls on s2 must still start behind it.
def test_stream_change_behind_a_call_that_settled_before_it_ran(eng, idle, streams):
    s1, s2 = streams[0], streams[1]
    short = ("resblock sc_5x5", "trunk b_like", "qtail nets")
    ref, ms = reference(idle, "long forward", lambda: trunk_forward_job(idle, "long"))
    print("the long trunk forward (n = %d) alone on the idle context: %.2f ms" % (LONG_N, ms))
    refs = [Sliced(infer_reference("stress", "f16x3", scales=False), ("rec",), 100, 130), ref] + [short_reference(idle, k) for k in short]
    makers = [lambda e: infer_job(100, 130, records=True), lambda e: trunk_forward_job(e, "long")] + [SHORT[k] for k in short]
    try:
        eng.set_activation_scales(False)         # with the calibrated scales these weights stay inside the fp16 range
        eng.load("Luma", 22, msbd_weights=_luma_weights("stress"))
        warm(eng, [m(eng) for m in makers])
        jobs = [m(eng) for m in makers]
        settled()
        before = eng.saturation_reruns()
        eng.set_stream(s1.cuda_stream)
        jobs[0].enqueue(eng)
        assert eng.saturation_reruns() == before, "the re-run is still to come"
        jobs[1].enqueue(eng)
        assert eng.saturation_reruns() > before, "the trunk call did not settle the pending re-run before it ran"
        eng.set_stream(s2.cuda_stream)
        for j in jobs[2:]:
            j.enqueue(eng)
        assert not s1.query(), "the trunk forward had finished before the short calls were enqueued: the case is too small"
        eng.synchronize()
    finally:
        eng.set_stream(0)
        eng.set_activation_scales(True)
        eng.load("Luma", 22, msbd_weights=_luma_weights("benign"))
    check(eng, list(zip(jobs, refs)))


# 6. the torch level: two trunk modules under two torch.cuda.stream blocks on one engine
def _modules():
    mods = []
    for name in ("long", "b_like"):
        c = trunk_case(name)[0] if name == "long" else T.make_case(T.EXACT["b_like"], 611, exact=False)
        seq = torch.nn.Sequential(*[R.reference_block(*blk) for blk in c["blocks"]]).cuda()
        mods.append((seq, up(c["x"]), up(c["g_y"]), bool(c["shape"][5])))
    return mods


def _clear(mods):
    for seq, x, _, _ in mods:
        x.grad = None
        x.requires_grad_()
        for p in seq.parameters():
            p.grad = None


def _grads(mods, ys):
    out = []
    for (seq, x, _, _), y in zip(mods, ys):
        out.append([y.detach().clone(), x.grad.clone()] + [p.grad.clone() for p in seq.parameters()])
    return out


def test_two_trunk_modules_under_two_torch_streams(eng, idle, streams):
    from pmp_vvc_tip2023_amd import trunk
    long_reference(idle)                         # prints the time of the first module's shape as a library call
    sa, sb = streams[0], streams[3]
    mods = _modules()
    cur = torch.cuda.current_stream()
    try:
        # one after the other with a synchronisation in between, on the same streams: the yardstick and the warm-up (twice: torch's
        # allocator then holds every block of both streams)
        for _ in range(2):
            _clear(mods)
            settled()
            ys = []
            for (seq, x, g, pool), s in zip(mods, (sa, sb)):
                with torch.cuda.stream(s):
                    y = trunk.trunk_of(eng, seq, x, pool=pool)
                    y.backward(g)
                torch.cuda.synchronize()
                ys.append(y)
            want = _grads(mods, ys)
        del ys, y
        _clear(mods)
        settled()
        ys = []
        for (seq, x, g, pool), s in zip(mods, (sa, sb)):
            with torch.cuda.stream(s):
                ys.append(trunk.trunk_of(eng, seq, x, pool=pool))
        assert not sa.query(), "the long forward had finished before the second module's was enqueued: the case is too small"
        torch.autograd.backward(ys, [g for _, _, g, _ in mods])
        cur.wait_stream(sa)
        cur.wait_stream(sb)
        got = _grads(mods, ys)
    finally:
        eng.set_stream(0)
    bad = {}
    for which, (a, b) in enumerate(zip(got, want)):
        for i, (t, w) in enumerate(zip(a, b)):
            k = int((_bits(t) != _bits(w)).sum())
            if k:
                bad["module %d, %s" % (which, ("y", "x.grad")[i] if i < 2 else "parameter %d's grad" % (i - 2))] = "%d of %d" % (k, t.numel())
    assert not bad, "differs from the two modules run one after the other: %s" % bad


# ---- (b) the walk ----------------------------------------------------------------------------------------------------------------------
POOL_N = 400


@functools.lru_cache(maxsize=None)
def label_case(which):
    return MS.valid_blocks(5, 1201, 1) if which == "msbt" else MS.tie_blocks(5, 1202)


def label_job(which):
    """pmp_msbt_labels_device / pmp_label_partition_device on five blocks of msbt_cases' label triples (cf 1)."""
    d = [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in label_case(which)]
    u8 = lambda *s: torch.full(s, 0xFF, dtype=torch.uint8, device="cuda")
    if which == "msbt":
        o = {"msbt": u8(5, 3, 16, 16), "status": u8(5)}
        return Job("msbt_labels", lambda e: e.msbt_labels_device(1, P(d[0]), P(d[1]), P(d[2]), 5, P(o["msbt"]), P(o["status"])), o, keep=d)
    o = {"hor": u8(5, 16, 16), "ver": u8(5, 16, 16), "status": u8(5)}
    return Job("label_partition", lambda e: e.label_partition_device(1, P(d[0]), P(d[1]), P(d[2]), 5, P(o["hor"]), P(o["ver"]), P(o["status"])),
               o, keep=d)


def trunk_unpack_job(e, name):
    """forward, backward and the unpacking of the saved x (index 0) of a trunk case."""
    j = trunk_job(e, name)
    dev, dense = j.keep, nan(*j.keep.x.shape)
    j._tensors["x_unpacked"] = dense
    both = j.enqueue
    j.enqueue = lambda e: (both(e), e.trunk_unpack_device(dev.shape, P(dev.saved), 0, P(dense)))
    return j


@functools.lru_cache(maxsize=None)
def val_labels(n):
    return V.labels(n, 7707)


def val_in_flight_job(lo, n):
    """pmp_infer_device into the caller's logits and, behind it with nothing in between, pmp_val_stats_device on those logits (no
    d_block_stats): the statistics are replayed if the inference call's range flag fires (api_labels.cpp: val_device_impl)."""
    d = torch.from_numpy(block_pool()[lo:lo + n]).cuda()
    lab = [torch.from_numpy(a).cuda() for a in val_labels(n)]
    o = {"qt": nan(n, 64), "bt": nan(n, 768), "dire": nan(n, 768), "stats": torch.full((20,), -1.0, dtype=torch.float64, device="cuda")}

    def enqueue(e):
        e.infer_device("Luma", 22, d.data_ptr(), None, None, n, P(o["qt"]), P(o["bt"]), P(o["dire"]))
        e.val_stats_device(22, P(o["qt"]), P(o["bt"]), P(o["dire"]), P(lab[0]), P(lab[1]), P(lab[2]), n, P(o["stats"]), None)
    return Job("infer + val_stats %d" % n, enqueue, o, keep=(d, lab))


def val_in_flight_reference(idle, kind, prec, scales, lo, n):
    """The idle inference context's logits of these blocks, and the idle training context's statistics of exactly those logits."""
    key = ("val", kind, prec, scales, lo, n)
    if key not in _REF:
        ref = infer_reference(kind, prec, scales)
        o = {k: ref[k][lo:lo + n].clone() for k in ("qt", "bt", "dire")}
        lab = [torch.from_numpy(a).cuda() for a in val_labels(n)]
        o["stats"] = torch.full((20,), -1.0, dtype=torch.float64, device="cuda")
        settled()
        idle.val_stats_device(22, P(o["qt"]), P(o["bt"]), P(o["dire"]), P(lab[0]), P(lab[1]), P(lab[2]), n, P(o["stats"]), None)
        idle.synchronize()
        _REF[key] = Job("idle", None, o)
    return _REF[key]


WALK_JOBS = {
    "resblock": {"identity": lambda e: block_job("identity"), "padded_cout": lambda e: block_job("padded_cout"), "sc_5x5": lambda e: block_job("sc_5x5")},
    "trunk": {"b_like": lambda e: trunk_unpack_job(e, "b_like"), "one_pool": lambda e: trunk_unpack_job(e, "one_pool")},
    "qtail": {"nets": lambda e: tail_job(e, "nets")},
    "stem": {"q_luma_one": lambda e: stem_job("q_luma_one"), "q_chroma": lambda e: stem_job("q_chroma")},
    "head": {"one_8x8": lambda e: head_job("one_8x8"), "b1_16x24": lambda e: head_job("b1_16x24")},
    "gate": {"1023": lambda e: gate_job(1023)},
    "train_loss": {"5": lambda e: loss_job(5), "17": lambda e: loss_job(17)},
    "labels": {"msbt": lambda e: label_job("msbt"), "partition": lambda e: label_job("partition")},
}
WALK_OPS = ["device", "device", "device", "host", "val_in_flight", "val_in_flight", "resblock_host"] + 2 * sorted(WALK_JOBS) + \
           ["weights", "chunk", "fusion", "overlap", "scales", "precision", "sync", "stream", "stream", "stream", "policy", "poison"]
WALK_STEPS = 80


def walk_plan(seed):
    """The walk of a seed, as data: [(op, its argument, the settings in force when it runs)].  No GPU needed."""
    rng = np.random.default_rng(seed)
    st = {"kind": "benign", "prec": "f16x3", "scales": True, "policy": "rerun"}
    plan = []
    for _ in range(WALK_STEPS):
        op, arg = str(rng.choice(WALK_OPS)), None
        fires = st["kind"] == "stress" and not st["scales"] and st["prec"] == "f16x3"
        if op in ("device", "host", "val_in_flight") and fires and st["policy"] == "ignore":
            op = "sync"                       # a context told to ignore a fired range flag keeps the clamped results: nothing to compare with
        if op == "device":
            n = int(rng.choice([1, 5, 37, 130]))
            arg = (int(rng.integers(0, POOL_N - n + 1)), n)
        elif op == "host":
            n = int(rng.choice([1, 6]))
            arg = (int(rng.integers(0, POOL_N - n + 1)), n)
        elif op == "val_in_flight":
            arg = (int(rng.choice([0, 211])), 37)
        elif op in WALK_JOBS:
            arg = str(rng.choice(sorted(WALK_JOBS[op])))
        elif op == "resblock_host":
            arg = str(rng.choice(["identity", "padded_cout"]))
        elif op == "weights":
            arg = st["kind"] = str(rng.choice(["benign", "trained", "stress"]))
        elif op == "chunk":
            arg = int(rng.choice([3, 64, 500, 4096]))
        elif op == "fusion":
            arg = int(rng.integers(0, 4))
        elif op in ("overlap", "scales"):
            arg = bool(rng.integers(0, 2))
            if op == "scales":
                st["scales"] = arg
        elif op == "precision":
            arg = st["prec"] = str(rng.choice(["f16x3", "f16x3", "fp32", "bf16x6"]))
        elif op == "stream":
            arg = int(rng.integers(0, 4))     # 0: the context's own, 1..3: torch streams
        elif op == "policy":
            arg = st["policy"] = str(rng.choice(["rerun", "ignore"]))
        elif op == "poison":
            arg = int(rng.choice([0, 2]))
        plan.append((op, arg, dict(st)))
    return plan


def records_of(hor, ver, q8, d8):
    n = hor.shape[0]
    return np.concatenate([hor.reshape(n, -1), ver.reshape(n, -1), q8.reshape(n, -1), d8.reshape(n, -1).view(np.uint8)], axis=1)


# by walk_plan(): each of these seeds walks through every op; between them they use all three weight sets, all three datapaths and both
# policies, and seed 15 has seven inference calls whose range flag fires
@pytest.mark.parametrize("seed", [1, 9, 15])
def test_random_training_api_walk_is_result_neutral(idle, streams, seed):
    """test_random_api_sequences_are_result_neutral's walk over the whole ABI: inference (device and host forms), labels, validation
    statistics on logits still in flight, losses, every training call (device forms, the ResidualBlock's host forms), with the stream,
    the weights, chunk, fusion, overlap, scales, datapath, saturation policy and workspace poisoning changed in between - and device
    calls left in flight across all of it.  Checked at each `sync`, with four calls in flight, and at the end."""
    from pmp_vvc_tip2023_amd import engine
    plan = walk_plan(seed)
    pool = block_pool()
    # everything the walk needs exists before its first call: jobs on buffers of their own, their idle references, the host calls' answers
    todo = []
    for op, arg, st in plan:
        job = ref = want = None
        iref = lambda: infer_reference(st["kind"], st["prec"], st["scales"])
        if op == "device":
            job, ref = infer_job(arg[0], arg[1], records=True), Sliced(iref(), ("rec",), *arg)
        elif op == "host":
            want = iref()["rec"][arg[0]:arg[0] + arg[1]].cpu().numpy()
        elif op == "val_in_flight":
            job, ref = val_in_flight_job(*arg), val_in_flight_reference(idle, st["kind"], st["prec"], st["scales"], *arg)
        elif op in WALK_JOBS:
            make = WALK_JOBS[op][arg]
            job, ref = make(idle), reference(idle, ("walk", op, arg), lambda: make(idle))[0]
        todo.append((op, arg, st, job, ref, want))
    e = engine.Engine(0, allow_synthetic_mtt=True)
    try:
        e.load("Luma", 22, msbd_weights=_luma_weights("benign"))
        # warm-up: every call once per datapath, settled - workspace, logit, scratch and staging buffers have their final size
        for prec in ("fp32", "bf16x6", "f16x3"):
            e.set_precision(prec)
            warm(e, [infer_job(0, 130, records=True), val_in_flight_job(0, 37)])
            e.infer_postprocess("Luma", 22, pool[:6])
        warm(e, [make(e) for fam in WALK_JOBS.values() for make in fam.values()])
        for name in ("identity", "padded_cout"):
            R.host_calls(e, block_case(name)[0])
        settled()
        in_flight, checked, last = [], 0, len(todo) - 1
        for step, (op, arg, st, job, ref, want) in enumerate(todo):
            if job is not None:
                job.enqueue(e)
                in_flight.append((job, ref, step, st))
            elif op == "host":
                got = records_of(*e.infer_postprocess("Luma", 22, pool[arg[0]:arg[0] + arg[1]]))
                assert np.array_equal(got, want), "step %d: host call differs under %s" % (step, st)
                checked += 1
            elif op == "resblock_host":
                c, table = block_case(arg)
                rf, rb, o = R.host_calls(e, c)
                assert rf == 0 and rb == 0, (step, e.lib.pmp_last_error(e.h))
                R.check_bits("step %d: host forms of %s" % (step, arg), o, table)
                checked += 1
            elif op == "weights":
                e.load("Luma", 22, msbd_weights=_luma_weights(arg))          # replacing a net settles the calls in flight first
            elif op == "chunk":
                e.set_chunk(arg)
            elif op == "fusion":
                e.set_fusion(arg)
            elif op == "overlap":
                e.set_overlap(arg)
            elif op == "scales":
                e.set_activation_scales(arg)
            elif op == "precision":
                e.set_precision(arg)
            elif op == "stream":
                e.set_stream(streams[arg - 1].cuda_stream if arg else 0)
            elif op == "policy":
                e.set_saturation_policy(arg)
            elif op == "poison":
                e._ck(e.lib.pmp_debug_poison_workspace(e.h, arg))
            if op == "sync" or len(in_flight) >= 4 or step == last:
                e.synchronize()                                              # the read point: nothing else has waited for the device
                for job, ref, at, s0 in in_flight:
                    bad = differing(job, ref)
                    assert not bad, "%s of step %d differs from the idle context's run in (tensor: elements) %s (settings then: %s)" % (job.name, at, bad, s0)
                for job, _, _, _ in in_flight:
                    if job.table:
                        job.table(e)
                    checked += 1
                in_flight = []
        assert checked >= 40
    finally:
        e.set_stream(0)
        e._ck(e.lib.pmp_debug_poison_workspace(e.h, 0))
        e.close()
