"""The single-tensor gains of oracle/range_cases.py, checked without a GPU through the float64 walk (oracle/layers64.py).

tests/test_gpu_range_sites.py trusts this table: each case must move only its own tensors, keep the nets' function (or change exactly
the logit it gains), and leave every other tensor well inside the fp16 range - otherwise a flag on the GPU could come from elsewhere."""
import os

import numpy as np
import pytest
import torch

from oracle import range_cases as R

COMPS = ("Luma", "Chroma")
_CACHE = {}


def _table(comp):
    if comp not in _CACHE:
        torch.set_num_threads(min(16, os.cpu_count() or 1))
        _CACHE[comp] = R.cases_for(comp)
    return _CACHE[comp]


def _walk_case(comp, case, s, drop=None):
    """The float64 walk of the gained nets; a net whose weights the case leaves alone is taken from the ungained walk."""
    cases, base, (wq, wb), x = _table(comp)
    gq, gb = case.apply(wq, wb, s, drop=drop)
    nets = ("q", "bd") if case.net == "qbd" else (case.net,)
    given = {k: v for k, v in base.items() if k.split("/")[0] not in nets}
    return R.walk(gq, gb, comp == "Luma", x, nets=nets, given=given)


def _logits(taps):
    q = taps["q/head"]
    h = [taps["bd/head%d" % k] for k in range(3)]
    return q, torch.stack([x[:, 0] for x in h], 1), torch.stack([x[:, 1] for x in h], 1)


def check_case(comp, case, exps=(0, 0, 0, 0, 0), drop=None):
    """-> list of problems (empty: the case does what the table says).  Walks at s_over; the run's tensors scale by exactly |s| (checked),
    so their stored maxima at s_under are s_under / s_over of those at s_over."""
    cases, base, _, _ = _table(comp)
    s = case.s_over
    got = _walk_case(comp, case, s, drop=drop)
    bad = []
    g = R.logit_gain(case, s)
    for nm, a, b, gk in zip(("qt", "bt", "dire"), _logits(got), _logits(base), (g["qt"], g["bt"], g["dire"])):
        gk = torch.as_tensor(np.broadcast_to(gk, (a.shape[1],)).copy()).view(1, -1, *([1] * (a.ndim - 2)))
        sgn = np.sign(s) if not case.preserving else 1.0
        want = b * torch.where(gk == 1.0, torch.ones_like(gk), gk * sgn)
        err = float((a - want).abs().max()) / max(float(want.abs().max()), 1e-30)
        if err > 1e-6:
            bad.append("%s: %s off by %.3g relative" % (case.name, nm, err))
    for n in R.tap_names(base) + [R.STEM_Q]:
        if n not in got:
            continue
        a = R.stored_amax(got, n, exps)
        if n in case.run:
            want = R._gained_amax(case, base, n, exps) * abs(s)
            if not case.preserving:        # the ungained channels of a logit plane are unchanged and far below the gained one
                want = max(want, R.stored_amax(base, n, exps))
            if abs(a - want) > 1e-6 * want:
                bad.append("%s: %s at %.6g, not |s| x %.6g" % (case.name, n, a, want / abs(s)))
            if (a > R.LIMIT) != (n in case.over):
                bad.append("%s: %s at %.6g (over: %s)" % (case.name, n, a, n in case.over))
            if a * abs(case.s_under / s) >= R.LIMIT and not R.fp32_stored(n, base):   # fp32 stores do not clamp
                bad.append("%s: %s at %.6g with s_under" % (case.name, n, a * abs(case.s_under / s)))
        elif a >= R.LIMIT / 4:
            bad.append("%s: %s outside the case at %.6g" % (case.name, n, a))
    if not any(n in case.over and not R.fp32_stored(n, base) for n in case.run) and any(not R.fp32_stored(n, base) for n in case.run):
        bad.append("%s: no split-2 tensor of the run crosses 65504" % case.name)
    return bad


def _ids():
    return [(comp, i) for comp in COMPS for i in range(len(R.build_cases(*R.base_weights(comp))))]


@pytest.mark.parametrize("comp,i", _ids(), ids=lambda p: str(p))
def test_case_moves_only_its_tensors(comp, i):
    """Function-preserving cases: logits within 1e-6 relative of the ungained nets; logit cases: exactly the gained logit times s.  The run's
    tensors scale by |s|, exactly the named ones cross 65504 at s_over and none at s_under, everything else stays below 65504 / 4."""
    case = _table(comp)[0][i]
    bad = check_case(comp, case)
    assert not bad, bad


_CHAIN = ("identity-shortcut chain trunk_M1.0..trunk_M2.3: every weight gain that reaches this tensor moves the whole chain by one factor "
          "(the identity shortcut carries it), so only the chain's largest tensors cross 65504 - it is driven to %.1f%% of the threshold "
          "there.  Its store is the conv_h2_kernel epilogue (conv_f16x3.hip, unfused in every mode) whose report the over-driven chain "
          "members and the single-tensor block cases exercise")
_Q12 = ("identity-shortcut run resblock_q1..resblock_q2: the gain of resblock_q1's output passes through resblock_q2's identity "
        "shortcut, so only the larger of the two crosses 65504 - this one is driven to %.1f%% of the threshold.  Both are stored by the "
        "conv_h2_kernel epilogue (unfused in every mode)")
# every tap that no case drives beyond 65504, with the reason; the table must match this list exactly (a new gap fails, and so does a
# listed tensor that a case now covers)
UNCOVERED = {
    "Luma": {"q/resblock_q2": _Q12, "bd/trunk_M1.0": _CHAIN, "bd/trunk_M1.3": _CHAIN, "bd/trunk_M1.4": _CHAIN, "bd/trunk_M1.5": _CHAIN,
             "bd/trunk_M2.0": _CHAIN},
    "Chroma": {"q/resblock_q1": _Q12, "bd/trunk_M1.0": _CHAIN, "bd/trunk_M1.1": _CHAIN, "bd/trunk_M1.2": _CHAIN, "bd/trunk_M1.3": _CHAIN,
               "bd/trunk_M1.4": _CHAIN, "bd/trunk_M1.5": _CHAIN, "bd/trunk_M2.0": _CHAIN, "bd/trunk_M2.1": _CHAIN},
}


def test_every_tap_is_covered():
    """Every tap of both nets and both components is a tensor of at least one case, and beyond 65504 in at least one - alone, or in a
    named joint case - except the tensors listed in UNCOVERED with their reason; nothing else is exempt."""
    counts = []
    for comp in COMPS:
        cases, base, _, _ = _table(comp)
        names = set(R.tap_names(base))
        ran = set(n for c in cases for n in c.run)
        assert names <= ran, "%s: no case covers %s" % (comp, sorted(names - ran))
        over = set(n for c in cases for n in c.over)
        assert R.STEM_Q in over
        never = names - over
        assert never == set(UNCOVERED[comp]), "%s: never over range but not listed: %s; listed but covered: %s" % (
            comp, sorted(never - set(UNCOVERED[comp])), sorted(set(UNCOVERED[comp]) - never))
        for n in sorted(never):
            c = next(c for c in cases if n in c.run)
            frac = R._gained_amax(c, base, n, (0,) * 5) * abs(c.s_over) / R.LIMIT
            assert frac < 1.0
            print("%s %s not over range: %s" % (comp, n, UNCOVERED[comp][n] % (100 * frac)))
        for net in ("q", "bd", "qbd"):
            counts.append("%s %s: %d" % (comp, net, sum(c.net == net for c in cases)))
        signs = {c.name[-1] for c in cases if not c.preserving}
        assert signs == {"+", "-"}
    print("range cases per net: " + ", ".join(counts))


def test_dropped_compensation_is_caught():
    """The check sees a mistake in the table: leaving out one consumer's 1/s changes the logits (and over-drives downstream)."""
    cases = _table("Luma")[0]
    for name, drop in (("q/resblock_q1..resblock_q2", "resblock_q3.left.0.weight"), ("bd/trunk_B2.0", "trunk_B2.1.shortcut.0.weight"),
                       ("bd/trunk_M1.0..trunk_M2.3", "trunk_Att1.1.left.2.weight")):
        case = next(c for c in cases if c.name == name)
        assert not check_case("Luma", case)
        bad = check_case("Luma", case, drop=drop)
        assert any("off by" in b for b in bad), (name, drop, bad)


def test_segment_cases_bracket_the_threshold_in_stored_units():
    """The five cases with non-zero exponents, one per MTT segment: walked with the exponents, the stored value (true x 2^-E) of the
    over-driven tensor crosses 65504 at s_over and not at s_under, and nothing else leaves 65504 / 4 (stored)."""
    cases, base, _, _ = _table("Luma")
    seg = R.segment_cases(cases, base)
    assert [R.segment(c.run[0]) for c in seg] == [0, 1, 2, 3, 4]
    for c in seg:
        assert R.SEGMENT_EXPS[R.segment(c.run[0])] > 0
        assert check_case("Luma", c, exps=R.SEGMENT_EXPS) == []
