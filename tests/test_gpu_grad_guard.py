"""GPU: the divergence guard (include/pmp.h, TRAINING STEP) - pmp_grad_guard_device, pmp_adam_step_guarded_device and optim.Adam's
max_grad_norm / skip_nonfinite.  Nothing here has a tolerance.

The census and the record, bit for bit against guard_cases' numpy restatement of the header's order (test_guard_cases_cpu.py holds
that restatement to the correctly rounded sum): one tensor and 97 (two launches: the tile numbering crosses the table), counts from
{1, 3, 255, 256, 257, 4095, 4096, 4097, 8193}, every tensor 4 bytes behind a 16-byte boundary or on one (both load paths), values whose
squares span 1e-60 .. 1e36, NaN and inf at a tile's first and last element, at the end of a ragged tail and mixed.  The scratch is
poisoned with NaNs first: the tiles' partials in it equal the restatement's, and the words behind pmp_grad_guard_scratch_bytes stay
poisoned.  The counters after a scripted sequence of taken, clipped and skipped calls.
The guarded Adam step, bit for bit against UNGUARDED pmp_adam_step_device calls: a skipped step writes nothing and still counts; a
clipped one equals the unguarded call fed g * coef (torch's float32 product, coef read back from the record); max_norm 0 on finite
gradients equals the unguarded call.  Tensors of 3, 65, 1025 (adam_cases') and 4097 elements.
The refusal matrix of `make traincheck`, through ctypes.  optim.Adam: the default's library calls are today's, counted through a
wrapped engine; a guarded optimiser's state_dict loads into torch.optim.Adam; step_taken and guard_state() follow the script."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import adam_cases as A
import guard_cases as G
import train_rig as R
from pmp_vvc_tip2023_amd import _lib

pytestmark = pytest.mark.gpu
eng = R.engine_fixture()
POISON = 0x7FF8DEADBEEF0001                                # a NaN as float64, and as two float32 words
TAIL = 5                                                  # words of scratch behind the call's


@functools.lru_cache(maxsize=None)
def reference(name, plant):
    """-> (the case's tensors, its census by guard_cases), computed once"""
    ts = G.table(name, plant)
    return ts, G.census(ts)


def bits(x):
    return np.asarray(x).tobytes()


class GuardDev:
    """A table on the device (off4: every tensor 4 bytes behind a 16-byte boundary in a NaN-filled allocation), a scratch poisoned
    with NaN patterns and TAIL words longer than asked for, a record of 0xFF bytes, counters at zero"""

    def __init__(self, e, tensors, off4=True):
        self.g = [R.Off4(R.up(a)) for a in tensors]
        self.d = [g.view if off4 else g.view.clone() for g in self.g]
        self.counts = [int(a.size) for a in tensors]
        self.bytes = e.grad_guard_scratch_bytes(self.counts)
        self.scratch = torch.full((self.bytes // 8 + TAIL,), POISON, dtype=torch.int64, device="cuda").view(torch.float64)
        self.record = torch.full((32,), 0xFF, dtype=torch.uint8, device="cuda")
        self.state = torch.zeros(6, dtype=torch.int64, device="cuda")
        R.torch_done()

    def run(self, e, max_norm=0.0, skip=False, state=True):
        e.grad_guard_device([R.P(a) for a in self.d], self.counts, R.P(self.scratch), R.P(self.record), R.P(self.state) if state else None,
                            max_norm=max_norm, skip_nonfinite=skip)
        e.synchronize()
        assert all(g.guards_intact() for g in self.g)
        return _lib.GuardRecord.from_buffer_copy(self.record.cpu().numpy().tobytes())

    def counters(self):
        s = _lib.GuardState.from_buffer_copy(self.state.cpu().numpy().tobytes())
        return {k: getattr(s, k) for k in G.STATE_KEYS}


def check_record(got, want, what):
    assert bits(np.float64(got.sumsq)) == bits(np.float64(want["sumsq"])), (what, got.sumsq, want["sumsq"])
    assert bits(np.float64(got.norm)) == bits(np.float64(want["norm"])), (what, got.norm, want["norm"])
    assert got.nonfinite == want["nonfinite"], what
    assert bits(np.float32(got.coef)) == bits(want["coef"]), (what, got.coef, want["coef"])
    assert got.action == want["action"], (what, got.action, want["action"])


@pytest.mark.parametrize("off4", [True, False], ids=["off4", "aligned"])
@pytest.mark.parametrize("name,plant", G.CASES, ids=["%s-%s" % c for c in G.CASES])
def test_census_and_record_bit_for_bit_from_a_poisoned_scratch(eng, name, plant, off4):
    ts, (sumsq, nonfinite, partials) = reference(name, plant)
    d = GuardDev(eng, ts, off4)
    tiles = len(partials)
    assert d.bytes == 16 * tiles and (len(ts) > _lib.PMP_ADAM_TABLE) == (name == "ninety_seven")
    norm = float(np.sqrt(sumsq))
    rules = G.RULES + ((norm, True), (norm / 4, False))           # norm == max_norm, and a plain clip
    for max_norm, skip in rules:
        got = d.run(eng, max_norm, skip)
        check_record(got, G.record(sumsq, nonfinite, max_norm, skip), (name, plant, max_norm, skip))
        words = d.scratch.cpu().numpy()
        assert bits(words[:tiles]) == bits(partials), "the tiles' partials, in the tiles' order"
        assert words[tiles:2 * tiles].view(np.int64).sum() == nonfinite
        assert (words[2 * tiles:].view(np.int64) == POISON).all(), "words behind the scratch's size were written"
    assert d.counters() == G.counters([G.record(sumsq, nonfinite, m, s) for m, s in rules])
    assert all(R.same_bits(R.num(a), t) for a, t in zip(d.d, ts)), "a gradient changed"


def test_without_counters_only_the_record_is_written(eng):
    ts, (sumsq, nonfinite, _) = reference("nine", "mixed")
    d = GuardDev(eng, ts)
    check_record(d.run(eng, 1.0, True, state=False), G.record(sumsq, nonfinite, 1.0, True), "no counters")
    assert d.counters() == G.counters([])


def test_same_bits_on_every_run_stream_and_context(eng):
    ts, _ = reference("ninety_seven", "none")

    def run(e, ts):
        d = GuardDev(e, ts)
        d.run(e, 1.0, True)
        return {"record": d.record.cpu().numpy(), "partials": d.scratch.cpu().numpy()[:d.bytes // 16]}
    R.same_bits_on_every_run_stream_and_context(eng, run, ts)


def test_counters_after_a_scripted_sequence_of_taken_clipped_and_skipped_calls(eng):
    small, big = np.full(300, 1e-3, np.float32), np.full(5000, 2.0, np.float32)
    bad, bad_big = small.copy(), big.copy()
    bad[7], bad_big[4999] = np.nan, -np.inf
    script = [(small, 1.0, True), (bad, 1.0, True), (bad, 1.0, True), (big, 1.0, True), (bad, 1.0, True), (bad_big, 1.0, True), (bad_big, 1.0, True),
              (bad, 1.0, False), (big, 0.0, True), (small, 1.0, True)]
    state = torch.zeros(6, dtype=torch.int64, device="cuda")
    want, actions = [], []
    for t, max_norm, skip in script:
        d = GuardDev(eng, [t])
        d.state = state
        actions.append(d.run(eng, max_norm, skip).action)
        s, n, _ = G.census([t])
        want.append(G.record(s, n, max_norm, skip))
    assert actions == [r["action"] for r in want] == [0, 1, 1, 2, 1, 3, 3, 0, 0, 0]
    got = d.counters()
    assert got == G.counters(want) and (got["steps"], got["skipped"], got["clipped"], got["run"], got["max_run"]) == (10, 5, 1, 0, 3)
    assert got["max_norm"] == max(r["norm"] for r in want) == float(np.sqrt(G.census([big])[0]))


# ---- the guarded Adam step
COUNTS = [3, 65, 1025, 4097]
KEYS = ("param", "m", "v")


class AdamPair:
    """The same tensors twice on the device: one set for guarded steps, one for unguarded ones"""

    def __init__(self, seed):
        self.t = A.tensors(COUNTS, seed, state=True)
        self.a = {k: [R.up(x) for x in self.t[k]] for k in KEYS}
        self.b = {k: [R.up(x) for x in self.t[k]] for k in KEYS}

    def ptrs(self, side, k):
        return [R.P(x) for x in side[k]]

    def snapshot(self, side):
        return {k: [R.num(x).copy() for x in side[k]] for k in KEYS}

    def same(self, x, y):
        return all(R.same_bits(a, b) for k in KEYS for a, b in zip(x[k], y[k]))


def guarded_step(e, pair, grads, step, max_norm, skip):
    """One guard call over grads and one guarded Adam step on pair.a -> the record"""
    d = GuardDev(e, [R.num(g) for g in grads], off4=False)
    d.d = grads
    rec = d.run(e, max_norm, skip)
    e.adam_step_guarded_device(pair.ptrs(pair.a, "param"), [R.P(g) for g in grads], pair.ptrs(pair.a, "m"), pair.ptrs(pair.a, "v"), COUNTS, step,
                               R.P(d.record))
    e.synchronize()
    return rec


def plain_step(e, pair, grads, step):
    e.adam_step_device(pair.ptrs(pair.b, "param"), [R.P(g) for g in grads], pair.ptrs(pair.b, "m"), pair.ptrs(pair.b, "v"), COUNTS, step)
    e.synchronize()


def test_a_skipped_step_writes_nothing_and_still_counts(eng):
    pair = AdamPair(51)
    grads = [[R.up(g) for g in A.tensors(COUNTS, 60 + i)["grad"]] for i in range(6)]
    grads[2][2][1000] = float("nan")                                  # step 3: one NaN in one tensor's gradient
    R.torch_done()
    for i in range(6):
        before = pair.snapshot(pair.a)
        kept = [R.num(g).copy() for g in grads[i]]
        rec = guarded_step(eng, pair, grads[i], i + 1, 0.0, True)
        assert rec.action == (1 if i == 2 else 0) and rec.nonfinite == (1 if i == 2 else 0)
        assert all(R.same_bits(R.num(g), k) for g, k in zip(grads[i], kept)), "the caller's gradients are not modified"
        if i == 2:
            assert pair.same(pair.snapshot(pair.a), before), "a skipped step wrote something"
        else:
            plain_step(eng, pair, grads[i], i + 1)                    # the same step NUMBER: the skipped step counted
            assert not pair.same(pair.snapshot(pair.a), before)
        assert pair.same(pair.snapshot(pair.a), pair.snapshot(pair.b)), "step %d" % (i + 1)
    assert all(np.isfinite(x).all() for k in KEYS for x in pair.snapshot(pair.a)[k])


def test_a_clipped_step_is_the_unguarded_step_on_g_times_coef(eng):
    pair = AdamPair(52)
    grads = [R.up(g) for g in A.tensors(COUNTS, 71, scale=3.0)["grad"]]
    sumsq = G.census([R.num(g) for g in grads])[0]
    norm = float(np.sqrt(sumsq))
    rec = guarded_step(eng, pair, grads, 4, norm / 3, True)
    assert rec.action == 2 and 0.3 < rec.coef < 0.34 and rec.coef == G.record(sumsq, 0, norm / 3)["coef"]
    coef = torch.tensor(rec.coef, dtype=torch.float32, device="cuda")
    scaled = [g * coef for g in grads]                                # one rounded float32 multiply each
    R.torch_done()
    plain_step(eng, pair, scaled, 4)
    assert pair.same(pair.snapshot(pair.a), pair.snapshot(pair.b))
    pair2 = AdamPair(52)                                              # and it differs from the step on the plain gradients
    plain_step(eng, pair2, grads, 4)
    assert not pair.same(pair.snapshot(pair.a), pair2.snapshot(pair2.b))


def test_max_norm_0_on_finite_gradients_is_the_unguarded_step(eng):
    pair = AdamPair(53)
    grads = [R.up(g) for g in A.tensors(COUNTS, 72)["grad"]]
    for max_norm, skip in ((0.0, False), (0.0, True), (1e30, True)):
        rec = guarded_step(eng, pair, grads, 2, max_norm, skip)
        assert rec.action == 0 and rec.coef == 1.0
        plain_step(eng, pair, grads, 2)
        assert pair.same(pair.snapshot(pair.a), pair.snapshot(pair.b))


# ---- refusals
def test_refusals_leave_record_counters_scratch_and_tensors_untouched(eng):
    t = A.tensors([5, 64, 257], 12, state=True)
    dev = {k: [R.up(a) for a in t[k]] for k in ("param", "grad", "m", "v")}
    counts = [5, 64, 257]
    own = torch.full((64,), POISON, dtype=torch.int64, device="cuda")               # scratch [0, 6), record [8, 12), counters [16, 22)
    R.torch_done()
    base = own.data_ptr()
    SC, REC, ST = base, base + 64, base + 128
    nan, inf = float("nan"), float("inf")
    G0, G1, G2 = (R.P(a) for a in dev["grad"])
    assert eng.grad_guard_scratch_bytes(counts) == 48
    nt = 3

    def guard(nm, which, ntensors=nt, null=(), entry=None, cnt=None, max_norm=1.0, scratch=SC, record=REC, state=ST):
        gp = [G0, G1, G2]
        for i, v in entry or ():
            gp[i] = v
        arr = None if "grad" in null else _lib.pointer_array(gp, nt)
        c = None if "count" in null else (C.c_int64 * nt)(*(cnt or counts))
        p = None if "p" in null else C.byref(_lib.GuardParams(max_norm, 1))
        return eng.lib.pmp_grad_guard_device(eng.h, p, ntensors, arr, c, None if "scratch" in null else scratch, None if "record" in null else record,
                                             state)

    def adam(nm, which, record=REC, step=1):
        arr = {k: _lib.pointer_array([R.P(a) for a in dev[k]], nt) for k in dev}
        p = C.byref(_lib.AdamParams(1e-3, 0.9, 0.999, 1e-8))
        return eng.lib.pmp_adam_step_guarded_device(eng.h, p, nt, arr["param"], arr["grad"], arr["m"], arr["v"], (C.c_int64 * nt)(*counts), step, record)

    tries = [("null " + k, "", "", dict(null=(k,))) for k in ("p", "grad", "count", "scratch", "record")] + \
            [("ntensors 0", "", "", dict(ntensors=0)), ("ntensors -1", "", "", dict(ntensors=-1)), ("a null gradient", "", "", dict(entry=[(1, None)])),
             ("a gradient two bytes off", "", "", dict(entry=[(1, G1 + 2)])), ("count 0", "", "", dict(cnt=[5, 0, 257])),
             ("count -1", "", "", dict(cnt=[5, -1, 257])), ("count 2^30", "", "", dict(cnt=[5, 1 << 30, 257])),
             ("max_norm -1", "", "", dict(max_norm=-1.0)), ("max_norm nan", "", "", dict(max_norm=nan)), ("max_norm inf", "", "", dict(max_norm=inf)),
             ("scratch 4 off", "", "", dict(scratch=SC + 4)), ("record 4 off", "", "", dict(record=REC + 4)), ("counters 4 off", "", "", dict(state=ST + 4)),
             ("scratch over a gradient", "", "", dict(scratch=G0)), ("record over a gradient", "", "", dict(record=G1)),
             ("counters over a gradient", "", "", dict(state=G2 + 1000)), ("record in the scratch", "", "", dict(record=SC + 40)),
             ("counters in the scratch", "", "", dict(state=SC + 32)), ("counters over the record", "", "", dict(state=SC + 88))]
    R.refuse_all(eng, tries, guard)
    P0, M2, V0 = R.P(dev["param"][0]), R.P(dev["m"][2]), R.P(dev["v"][0])
    tries = [("step 0", "", "", dict(step=0)), ("null record", "", "", dict(record=None)), ("record 4 off", "", "", dict(record=REC + 4)),
             ("record over a param", "", "", dict(record=P0)), ("record over a gradient", "", "", dict(record=G1)),
             ("record over an m", "", "", dict(record=M2 + 1000)), ("record over a v", "", "", dict(record=V0))]
    R.refuse_all(eng, tries, adam)
    assert (own.cpu().numpy() == POISON).all(), "a refused call wrote to scratch, record or counters"
    assert all(R.same_bits(R.num(a), src) for k in dev for a, src in zip(dev[k], t[k])), "a refused call wrote to a tensor"
    # the same calls, unharmed, are accepted: right behind one another too
    own[16:22] = 0
    R.torch_done()
    assert guard("", "") == 0 and guard("", "", record=SC + 48, state=SC + 80) == 0 and adam("", "") == 0
    eng.synchronize()
    assert not all(R.same_bits(R.num(a), src) for a, src in zip(dev["param"], t["param"]))


# ---- optim.Adam
class Counting:
    """An engine whose library calls of a step are counted"""
    NAMES = ("adam_step_device", "grad_guard_device", "adam_step_guarded_device")

    def __init__(self, engine):
        self.__dict__["inner"], self.__dict__["calls"] = engine, {k: 0 for k in self.NAMES}

    def __getattr__(self, name):
        v = getattr(self.inner, name)
        if name not in self.NAMES:
            return v

        def counted(*a, **k):
            self.calls[name] += 1
            return v(*a, **k)
        return counted

    def __setattr__(self, name, value):
        setattr(self.inner, name, value)


def test_optim_adam_defaults_make_todays_calls_and_the_guarded_one_follows_the_script(eng):
    from pmp_vvc_tip2023_amd import optim
    t = A.tensors(COUNTS, 31)
    grads = [A.tensors(COUNTS, 80 + i, scale=3.0)["grad"] for i in range(6)]
    bad = [g.copy() for g in grads[1]]
    bad[3][4096] = np.inf
    script = [grads[0], bad, bad, grads[3], bad, grads[5]]
    norms = [float(np.sqrt(G.census(g)[0])) for g in script]
    max_norm = 0.5 * min(norms)                                       # every taken step is clipped
    ce = Counting(eng)
    ps, qs = [torch.nn.Parameter(R.up(a)) for a in t["param"]], [torch.nn.Parameter(R.up(a)) for a in t["param"]]
    plain, guarded = optim.Adam(ce, ps, lr=2e-3), optim.Adam(ce, qs, lr=2e-3, max_grad_norm=max_norm, skip_nonfinite=True)
    assert not plain.guarded and plain.step_taken is None and guarded.guard_record() is None and guarded.guard_state()["steps"] == 0
    try:
        for p, g in zip(ps, script[0]):
            p.grad = R.up(g)
        plain.step()
        plain.step()
        assert ce.calls == {"adam_step_device": 2, "grad_guard_device": 0, "adam_step_guarded_device": 0}, "the default's calls are today's"
        taken, want = [], []
        for i, gs in enumerate(script):
            for q, g in zip(qs, gs):
                q.grad = R.up(g)
            before = [q.detach().clone() for q in qs]
            guarded.step()
            assert guarded.step_taken.is_cuda and guarded.step_taken.dtype == torch.bool
            taken.append(bool(guarded.step_taken))
            assert all(torch.equal(q.detach(), b) for q, b in zip(qs, before)) == (not taken[-1])
            s, n, _ = G.census(gs)
            want.append(G.record(s, n, max_norm, True))
            rec = guarded.guard_record()
            assert (rec["sumsq"], rec["norm"], rec["nonfinite"], rec["action"]) == (want[-1]["sumsq"], want[-1]["norm"], want[-1]["nonfinite"], want[-1]["action"])
            assert rec["coef"] == float(want[-1]["coef"]) and rec["skip"] == (not taken[-1]) and rec["clip"]
        torch.cuda.synchronize()
        assert ce.calls == {"adam_step_device": 2, "grad_guard_device": 6, "adam_step_guarded_device": 6}, "one guard call and one Adam call a step"
        assert taken == [True, False, False, True, False, True]
        state = guarded.guard_state()
        assert state == G.counters(want) and (state["steps"], state["skipped"], state["clipped"], state["max_run"]) == (6, 3, 3, 2)
        assert all(torch.isfinite(q).all() for q in qs)
        # a skipped step still counts; the state loads into torch's optimiser, the counters are not in it
        sd = guarded.state_dict()
        assert [float(sd["state"][i]["step"]) for i in range(4)] == [6.0] * 4 and sorted(sd["state"][0]) == ["exp_avg", "exp_avg_sq", "step"]
        assert "guard" not in sd and all("guard" not in k and "max_grad_norm" not in k for k in sd["param_groups"][0])
        topt = torch.optim.Adam([torch.nn.Parameter(q.detach().cpu().clone()) for q in qs], foreach=False)
        topt.load_state_dict(sd)
        assert topt.param_groups[0]["lr"] == 2e-3
        for cp, q in zip(topt.param_groups[0]["params"], qs):
            assert R.same_bits(topt.state[cp]["exp_avg"].numpy(), R.num(guarded.state[q]["exp_avg"]))
        # the counters put back into a fresh optimiser go on from where they were
        again = optim.Adam(ce, qs, lr=2e-3, max_grad_norm=max_norm, skip_nonfinite=True)
        again.load_guard_state(state)
        assert again.guard_state() == state
        again.load_state_dict(sd)
        again.step()
        assert again.guard_state() == G.counters([want[-1]], state)
    finally:
        eng.set_stream(0)
