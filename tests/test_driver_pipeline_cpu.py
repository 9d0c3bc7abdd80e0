"""CPU: the driver's pieces (inference_qbd.py) against recording fakes - the pass schedule of run_sequence, the pinned double buffer
of ShardedSink, the release after a failure, the Time_Sta writer.  No GPU, no torch device."""
from concurrent.futures import ThreadPoolExecutor
from types import SimpleNamespace

import numpy as np
import pytest

from pmp_vvc_tip2023_amd import emit, inference_qbd as D, parallel

P3 = [("Luma", 22), ("Luma", 37), ("Chroma", 22)]


class FakeEngine:
    """Records what the driver asks of the engine; 'infers' records that name their pass."""

    def __init__(self, log=None):
        self.log, self.provenance, self.closed = ([] if log is None else log), {}, 0

    def load(self, comp, qp):
        self.log.append(("load", comp, qp))

    def check_available(self, comp, qp):
        pass

    def saturation_reruns(self):
        return 0

    def output_block_yuv(self, y, u, v, bitdepth):
        n = y.shape[0] * (y.shape[1] // 64) * (y.shape[2] // 64)
        return np.zeros((n, 68, 68), np.uint8), np.zeros((n, 34, 34), np.uint8), np.zeros((n, 34, 34), np.uint8)

    def infer_postprocess(self, comp, qp, by, bu, bv):
        n = by.shape[0]
        self.log.append(("infer", comp, qp, n))
        return (np.full((n, 16, 16), qp, np.uint8), np.zeros((n, 16, 16), np.uint8), np.zeros((n, 8, 8), np.uint8),
                np.zeros((n, 3, 16, 16), np.int8))

    def close(self):
        self.closed += 1


class FakeSource:
    lookahead, n = True, 1

    def __init__(self, log):
        self.log = log

    def enqueue(self, comp, qp):
        self.log.append(("enqueue", comp, qp))
        return comp, qp

    def collect(self, handle):
        self.log.append(("collect",) + handle)
        return handle


class FakeSink:
    def __init__(self, log):
        self.log = log

    def put(self, k, save_path, seq, records):
        assert save_path.endswith("%s_%s_QP%d_PartitionMat.txt" % ((seq.stem,) + records))
        self.log.append(("put",) + records)

    def end_sequence(self):
        self.log.append(("end_sequence",))


def one_block_sequence():
    return D.Sequence("S", "S_64x64_30", 64, 64, 1, False, 1, 1, 0, 1, 0, 1)


def schedule_of(passes):
    log = []
    job = D.Job(0, 1, FakeEngine(log))
    D.run_sequence(job, 0, one_block_sequence(), FakeSource(log), FakeSink(log), passes, "out", D.TimeSta(1), D.Stages())
    return log


def test_run_sequence_schedule_of_three_passes():
    p0, p1, p2 = P3
    assert schedule_of(P3) == [
        ("load",) + p0, ("enqueue",) + p0, ("load",) + p1,
        ("collect",) + p0, ("enqueue",) + p1, ("load",) + p2, ("put",) + p0,
        ("collect",) + p1, ("enqueue",) + p2, ("put",) + p1,
        ("collect",) + p2, ("put",) + p2,
        ("end_sequence",)]


def test_run_sequence_without_a_pass_and_with_one():
    assert schedule_of([]) == [("end_sequence",)]
    p0 = P3[0]
    assert schedule_of([p0]) == [("load",) + p0, ("enqueue",) + p0, ("collect",) + p0, ("put",) + p0, ("end_sequence",)]


class FakeEmitter:
    """emit.ShardEmitter's phases, recorded.  finish(p) checks what the emitter's contract promises it: the array given to start()
    still holds the same bytes.  Once `dead` is set - the job has failed - any collective phase fails the test."""

    def __init__(self, *a, **kw):
        self.pool, self.log, self.dead = ThreadPoolExecutor(max_workers=1), [], False

    def start(self, path, frames, height, width, g_lo, g_hi, rec, binary=False):
        self.log.append(("start", path))
        return SimpleNamespace(path=path, rec=rec, given=rec.tobytes())

    def finish(self, p):
        assert not self.dead, "finish() after the failure"
        assert p.rec.tobytes() == p.given, "%s: the records changed between start() and finish()" % p.path
        self.log.append(("finish", p.path))
        p.rec = None

    def drain(self):
        assert not self.dead, "drain() after the failure"
        self.log.append(("drain",))

    def close(self):
        self.drain()
        self.pool.shutdown(wait=True)


class UnpinnedPool:
    """PinnedPool's take() without page-locking (which needs a GPU runtime): the double buffer's logic is the same."""

    def take(self, nbytes):
        import torch
        return torch.empty(max(int(nbytes), 1), dtype=torch.uint8)


@pytest.mark.parametrize("kind", ["host arrays", "tensors through the slots"])
def test_sharded_sink_never_rewrites_a_slot_before_its_finish(kind):
    """Five passes with distinct records, in order: finish() runs once per pass, for pass k-1 before start() of pass k+1 (in fact
    before start() of pass k), and at every finish() the emitter's array still holds what start() was given.  The tensor case goes
    through the two reused slots, as device records do."""
    import torch
    em = FakeEmitter()
    sink = D.ShardedSink(em, UnpinnedPool(), D.Stages())
    seq, want = one_block_sequence(), []
    for k in range(5):
        rec = np.full((3, parallel.RECORD), k + 1, np.uint8)
        sink.put(k, "f%d" % k, seq, rec if kind == "host arrays" else torch.from_numpy(rec))
        want += ([("finish", "f%d" % (k - 1))] if k else []) + [("start", "f%d" % k)]
        assert em.log == want
    sink.end_sequence()
    assert em.log == want + [("finish", "f4"), ("drain",)]
    assert sink.busy == [False, False]
    # the rule is asserted where it lives: a pass may not take a slot whose last pass has not been finished
    sink.put(0, "g0", seq, np.zeros((3, parallel.RECORD), np.uint8))
    with pytest.raises(AssertionError, match="slot 0"):
        sink.put(2, "g2", seq, np.zeros((3, parallel.RECORD), np.uint8))
    sink.abandon()


def tiny_job(tmp_path, monkeypatch, emit_mode):
    """A one-sequence job (one 64x64 frame, three passes, host blocks) on a fake engine: (args, job, fake emitter or None, writes)."""
    inp = tmp_path / "in"
    inp.mkdir()
    (inp / "T_64x64_30.yuv").write_bytes(bytes(64 * 64 * 3 // 2))
    (inp / "table.txt").write_text("T,T_64x64_30.yuv,64,64,1,30\n#end!!!!\n")
    (inp / "T.cfg").write_text("InputFile : T_64x64_30.yuv\nInputBitDepth : 8\n")
    args = D.build_parser().parse_args(["--inputDir", str(inp), "--outDir", str(tmp_path / "out"), "--seqTable", "table.txt", "--cfgDir", str(inp),
                                        "--ssRatio", "1", "--seqNum", "1", "--qps", "22,27,32", "--comps", "Luma", "--emit", emit_mode])
    job = D.Job(0, 1, FakeEngine())
    emitters, writes = [], []
    monkeypatch.setattr(D, "open_job", lambda a: job)
    monkeypatch.setattr(emit, "ShardEmitter", lambda *a, **kw: emitters.append(FakeEmitter()) or emitters[-1])
    monkeypatch.setattr(D, "_emit", lambda rec, path, *a: writes.append((path, int(rec[0, 0]))))
    return args, job, emitters, writes


@pytest.mark.parametrize("emit_mode", ["sharded", "gather"])
def test_job_on_a_fake_engine_ends_in_todays_order(tmp_path, monkeypatch, emit_mode):
    args, job, emitters, writes = tiny_job(tmp_path, monkeypatch, emit_mode)
    st = D.inference_VVC_seqs(args)
    assert st is D.LAST_STAGES and (st.passes, st.blocks) == (3, 3) and job.eng.closed == 1
    assert [e for e in job.eng.log if e[0] == "infer"] == [("infer", "Luma", q, 1) for q in (22, 27, 32)]
    assert job.reader.pool._shutdown
    if emit_mode == "sharded":
        names = [str(tmp_path / "out" / "0000" / "PartitionMat" / ("T_64x64_30_Luma_QP%d_PartitionMat.txt" % q)) for q in (22, 27, 32)]
        assert emitters[0].log == [("start", names[0]), ("finish", names[0]), ("start", names[1]), ("finish", names[1]), ("start", names[2]),
                                   ("finish", names[2]), ("drain",), ("drain",)]
        assert emitters[0].pool._shutdown
    else:
        assert [q for _, q in writes] == [22, 27, 32] and job.sink.writers._shutdown
    rows = (tmp_path / "out" / "0000" / "Time_Sta_0_1.txt").read_text().strip().split("\n")
    assert len(rows) == 4 and all(r.count(",") == 5 for r in rows)


@pytest.mark.parametrize("emit_mode", ["sharded", "gather"])
def test_a_failing_put_releases_what_the_process_owns_without_a_collective(tmp_path, monkeypatch, emit_mode):
    args, job, emitters, writes = tiny_job(tmp_path, monkeypatch, emit_mode)
    boom = RuntimeError("no space left on device")
    cls = D.ShardedSink if emit_mode == "sharded" else D.GatherSink
    real_put = cls.put

    def put(self, k, save_path, seq, records):
        if k == 1:
            for em in emitters:
                em.dead = True
            monkeypatch.setattr(parallel, "all_reduce_sum", lambda *a, **kw: pytest.fail("a collective after the failure"))
            raise boom
        real_put(self, k, save_path, seq, records)
    monkeypatch.setattr(cls, "put", put)
    with pytest.raises(RuntimeError) as e:
        D.inference_VVC_seqs(args)
    assert e.value is boom
    assert job.eng.closed == 1 and job.reader.pool._shutdown
    if emit_mode == "sharded":
        assert emitters[0].pool._shutdown and [x[0] for x in emitters[0].log] == ["start"]      # pass 0 started, never finished or drained
    else:
        assert job.sink.writers._shutdown
    assert not (tmp_path / "out" / "0000" / "Time_Sta_0_1.txt").exists()


def test_time_sta_has_the_references_shape(tmp_path):
    """Inference_QBD.py:243-253: four QP rows per sequence, five comma-terminated numbers each: block, net Luma, net Chroma, post
    Luma, post Chroma - Luma in column 0 whatever order --comps lists the components in."""
    sta = D.TimeSta(2)
    sta.block[:] = [0.5, 1.5]
    for si in range(2):
        for comp in ("Chroma", "Luma"):                          # as --comps Chroma,Luma runs them
            for qp in D.QPS:
                qi, ci = D.TimeSta.cell(comp, qp)
                sta.net[si, qi, ci] = 100 * si + qp + (0.25 if comp == "Chroma" else 0.0)
                sta.post[si, qi, ci] = -(100 * si + qp) - (0.25 if comp == "Chroma" else 0.0)
    path = tmp_path / "Time_Sta_0_2.txt"
    sta.write(str(path))
    text = path.read_text()
    rows = text.split("\n")
    assert rows.pop() == "" and len(rows) == 8 and all(r.endswith(",") and r.count(",") == 5 for r in rows)
    got = [[float(x) for x in r.split(",")[:5]] for r in rows]
    want = [[b, 100 * si + qp, 100 * si + qp + 0.25, -(100 * si + qp), -(100 * si + qp) - 0.25]
            for si, b in enumerate((0.5, 1.5)) for qp in D.QPS]
    assert got == want
    assert text.startswith("0.5,22.0,22.25,-22.0,-22.25,\n")        # str() of each number, as the reference writes them
    assert sta.total() == pytest.approx(sum(sum(r) for r in want) - 3 * (0.5 + 1.5))
    # the same through the pass loop: Chroma first on the command line still lands in column 1
    sta = D.TimeSta(1)
    D.run_sequence(D.Job(0, 1, FakeEngine()), 0, one_block_sequence(), FakeSource([]), FakeSink([]), [("Chroma", 37), ("Luma", 37)], "out", sta, D.Stages())
    assert (sta.net[0, 3] > 0).all() and (sta.net[0, :3] == 0).all() and D.TimeSta.cell("Luma", 37) == (3, 0)
