"""The convolution kernel instantiations the product library compiles against the table in oracle/conv_cases.py (no GPU needed): every
conv_h2 / conv_x6 / conv_mfma kernel symbol in the device code of libpmp_hip.so is in INSTANTIATIONS and every entry is a symbol, so a new
or removed instantiation fails here until the table says which cases reach it or why none can.  The case table's predicted dispatch
(expected_kernels, checked against the launches on the GPU by tests/test_gpu_conv_sweep.py) reaches exactly the entries marked reachable."""
import re

from cases_common import LIB, kernel_symbols
from oracle import conv_cases as CC

_SYM = re.compile(r"_ZN3pmp\d+(conv_h2_kernel|conv_x6_kernel|conv_mfma_kernel)I((?:L[ib]\d+E)+)E")


def test_instantiation_table_matches_the_library():
    syms = kernel_symbols(LIB, _SYM)
    assert syms, "no convolution kernel symbols found in " + LIB
    table = set(CC.INSTANTIATIONS)
    assert syms == table, "in the library, not in the table: %s; in the table, not in the library: %s" % (
        sorted(syms - table), sorted(table - syms))
    for name, why in CC.INSTANTIATIONS.items():
        assert why is None or (isinstance(why, str) and len(why) > 20), name


def test_case_table_reaches_every_reachable_instantiation():
    cases = CC.cases()
    assert 300 <= len(cases) <= 400 and len({c["id"] for c in cases}) == len(cases)
    reached = {k for c in cases for fusion in (False, True) for k in CC.expected_kernels(c, fusion)}
    reachable = {k for k, v in CC.INSTANTIATIONS.items() if v is None} | set(CC.FUSED)
    assert reached == reachable, (sorted(reachable - reached), sorted(reached - reachable))
    # the spans the sweep promises
    assert {c["n"] for c in cases} == {1, 2, 5}
    assert {(c["h"], c["w"]) for c in cases} == set(CC.MAPS)
    assert {c["cin"] // 16 for c in cases} >= {1, 2, 3, 5, 8}
    assert {c["wdist"] for c in cases if c["dp"] == "f16x3"} == set(CC.WDISTS)
    assert {c["xdist"] for c in cases} == set(CC.XDISTS)
    for dp in CC.DATAPATHS:
        sub = [c for c in cases if c["dp"] == dp]
        assert any(c["gate"] for c in sub) and any(c["pool"] for c in sub) and any(c["out_f32"] for c in sub), dp
    assert any(c["exp_x"] != 0 and c["gate"] and c["exp_out"] != c["exp_x"] for c in cases if c["dp"] == "f16x3")


def test_weight_edges_reach_the_scale_edges():
    """The f16x3 weight edges do what their names say: a negative k, the cap of 24, a shortcut that sets (or not) the shared k2, k = 0 for
    an all-zero tensor, max |S*w| = 4096 exactly for powers of two."""
    def first(wd):
        c = next(c for c in CC.cases() if c["dp"] == "f16x3" and c["wdist"] == wd and c["cin"] != c["cout"])
        return CC.tensors(c)
    _, w0, w2, wsc, _ = first("w0_big")
    assert CC.h2_scale_exp(w0) < 0
    _, w0, w2, wsc, _ = first("cap")
    assert CC.h2_scale_exp(w0) == 24 and abs(w0).max() * 2.0 ** 24 < 4096
    for wd, d in (("sc+12", 12), ("sc+18", 18), ("sc-12", -12), ("sc-18", -18)):
        _, w0, w2, wsc, _ = first(wd)
        k0, k2 = CC.rb_scale_exps(w0, w2, wsc)
        assert abs(min(24, CC.h2_scale_exp(w2) - d) - CC.h2_scale_exp(wsc)) <= 1, wd        # (the cap of 24 may clip ksc)
        assert k2 == min(CC.h2_scale_exp(w2), CC.h2_scale_exp(wsc)), wd
    _, w0, w2, wsc, _ = first("zero_w0")
    assert not w0.any() and CC.h2_scale_exp(w0) == 0
    _, w0, w2, wsc, _ = first("pow2")
    assert abs(w0).max() * 2.0 ** CC.h2_scale_exp(w0) == 4096
