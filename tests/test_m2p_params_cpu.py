"""CPU: the Map2Partition thresholds (include/pmp.h: pmp_partition_params) - the host-only parser and its domain check, the
driver's --m2p / --m2pChroma flags, and the reference-made fixture G10 (tests/golden/g10_m2p_params.npz) against the older fixtures
and the pinned oracle at the defaults.  The GPU side is tests/test_gpu_m2p_params.py."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, golden
import m2p_params_cases as K
from pmp_vvc_tip2023_amd import _lib, engine as E

KEYS = E.PARAM_KEYS


@pytest.fixture(scope="module")
def lib():
    if not os.path.isfile(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.load()


def parse(lib, spec, base=None):
    """-> (rc, dict after the call); `base` (dict) is what *inout holds before."""
    b = dict(E.DEFAULT_PARTITION_PARAMS, **(base or {}))
    p = _lib.PartitionParams()
    for i, k in enumerate(KEYS[:5]):
        p.lamb[i] = b[k]
    p.thd = b["thd"]
    rc = lib.pmp_parse_partition_params(spec.encode() if isinstance(spec, str) else spec, C.byref(p))
    return rc, E.params_dict(p)


def test_exports(lib):
    for name in ("pmp_set_partition_params", "pmp_get_partition_params", "pmp_parse_partition_params"):
        assert hasattr(lib, name)
    assert C.sizeof(_lib.PartitionParams) == 48


def test_parse_round_trips(lib):
    d = E.DEFAULT_PARTITION_PARAMS
    assert parse(lib, "") == (0, d)
    assert parse(lib, ",") == (0, d)
    for name, vals in K.SETS.items():
        spec = ",".join("%s=%r" % (k, v) for k, v in zip(KEYS, vals))
        rc, got = parse(lib, spec)
        assert rc == 0, (name, lib.pmp_last_error(None))
        assert [got[k] for k in KEYS[:5]] == list(vals[:5])
        assert got["thd"] == float(np.float32(vals[5]))                # stored as float32: numpy compares in float32
        # printed back with repr and parsed again: the same numbers
        again = parse(lib, ",".join("%s=%r" % kv for kv in got.items()))
        assert again == (0, got)
    # a subset on top of what *inout holds; repeated keys: the last wins; spaces around items
    assert parse(lib, "lamb1=0.6", {"lamb2": 0.9})[1] == dict(d, lamb1=0.6, lamb2=0.9)
    assert parse(lib, "lamb1=0.6,lamb1=0.55")[1]["lamb1"] == 0.55
    assert parse(lib, " lamb4 = 0.25 , thd=0.7 ")[1] == dict(d, lamb4=0.25, thd=float(np.float32(0.7)))
    assert parse(lib, "lamb3=1e0,lamb2=0x1p-1")[1] == dict(d, lamb3=1.0, lamb2=0.5)
    # the Python helper goes through the same parser
    assert E.parse_partition_params("lamb5=0.8") == dict(d, lamb5=0.8)
    assert E.parse_partition_params("thd=0.45", {"lamb1": 0.5}) == dict(d, lamb1=0.5, thd=float(np.float32(0.45)))


@pytest.mark.parametrize("spec", [
    "lamb1=0", "lamb1=1", "lamb2=0", "lamb2=1e300", "lamb3=0", "lamb3=7.5", "lamb4=0", "lamb4=1", "lamb5=0.67", "lamb5=1",
    "thd=2", "thd=1e-30", "thd=0.5", "lamb1=-0", "lamb5=0.6700000000000000001",
])
def test_domain_edges_accepted(lib, spec):
    rc, got = parse(lib, spec)
    assert rc == 0, lib.pmp_last_error(None)
    k, v = spec.split("=")
    assert got[k] == (float(np.float32(float(v))) if k == "thd" else float(v))


@pytest.mark.parametrize("spec", [
    "lamb1=-1e-300", "lamb1=1.0000000000000002", "lamb2=-1e-300", "lamb3=-0.5", "lamb4=-0.1", "lamb4=1.0000000000000002",
    "lamb5=0.6699999999999999", "lamb5=0.2", "lamb5=1.0000000000000002", "thd=0", "thd=-0.5", "thd=2.0000001", "thd=1e-50",
    "lamb1=nan", "lamb2=inf", "lamb3=-inf", "lamb4=NAN", "lamb5=Infinity", "thd=nan", "thd=inf", "lamb2=1e309",
    "lamb6=0.5", "lamb0=0.5", "thd2=0.5", "LAMB1=0.5", "lamb=0.5", "x=1",
    "lamb1", "lamb1=", "=0.5", "lamb1=0.5x", "lamb1=0.5 0.6", "lamb1=0.5;lamb2=0.6", "lamb1=0.6,bogus",
])
def test_domain_edges_rejected(lib, spec):
    before = {"lamb1": 0.6, "thd": 0.25}
    b = dict(E.DEFAULT_PARTITION_PARAMS, **before)
    rc, got = parse(lib, spec, before)
    assert rc == -1, spec
    assert got == dict(b, thd=float(np.float32(0.25)))                    # *inout untouched
    assert lib.pmp_last_error(None)
    with pytest.raises(_lib.PmpError):
        E.parse_partition_params(spec)


def test_parse_null_arguments(lib):
    p = _lib.PartitionParams()
    assert lib.pmp_parse_partition_params(None, C.byref(p)) == -1
    assert lib.pmp_parse_partition_params(b"lamb1=0.5", None) == -1


def test_context_calls_need_a_context(lib):
    p = _lib.PartitionParams()
    assert lib.pmp_set_partition_params(None, 0, C.byref(p)) == -1
    assert lib.pmp_get_partition_params(None, 0, C.byref(p)) == -1


def test_driver_flags(tmp_path):
    """--m2p / --m2pChroma go through the C parser before any GPU work: a bad spec ends the driver with a message."""
    from pmp_vvc_tip2023_amd import inference_qbd as D
    a = D.build_parser().parse_args(["--m2p", "lamb1=0.6,thd=0.7", "--m2pChroma", "lamb5=0.9"])
    got = D.partition_params(a)
    assert got["Luma"] == dict(E.DEFAULT_PARTITION_PARAMS, lamb1=0.6, thd=float(np.float32(0.7)))
    assert got["Chroma"] == dict(got["Luma"], lamb5=0.9)
    assert D.partition_params(D.build_parser().parse_args([])) == {"Luma": E.DEFAULT_PARTITION_PARAMS, "Chroma": E.DEFAULT_PARTITION_PARAMS}
    r = subprocess.run([sys.executable, "-m", "pmp_vvc_tip2023_amd.inference_qbd", "--m2p", "lamb5=0.5", "--outDir", str(tmp_path)],
                       cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "lamb5" in r.stderr and not (tmp_path / "0000").exists()


def test_g10_defaults_reproduce_g3_g9_and_the_oracle(oracle_lib):
    """The reference-made G10 at the defaults equals G3 / G9 where eli_structual_error leaves the QT map alone, and the pinned oracle
    (which has the defaults built in) everywhere, on eli_structual_error's output."""
    g10 = golden("g10_m2p_params.npz")
    assert list(g10["set_names"]) == list(K.SETS) and np.array_equal(g10["set_values"], np.array(list(K.SETS.values())))
    g3, g9 = golden("g3_m2p.npz"), golden("g9_m2p_seeded.npz")
    n = 0
    for cf in (1, 2):
        for src, qt, bt, dire in K.inputs(cf, 0.5):
            h, v, d = K.expected(g10, "defaults", src, cf)
            fixed = oracle_lib.eli_structural_error(qt).reshape(-1, 8, 8)
            oh, ov, od, _ = oracle_lib.map_to_partition(fixed, bt, dire, cf)
            assert np.array_equal(h, oh) and np.array_equal(v, ov) and np.array_equal(d, od), (src, cf)
            if src.startswith("g3"):
                t = src[2:]
                sl = dict(K.G3_SLICES)[t]
                same = np.all(fixed == qt, axis=(1, 2))
                for a, k in zip((h, v, d), ("hor", "ver", "dout")):
                    assert np.array_equal(a[same], g3["%s_%s_cf%d" % (t, k, cf)][sl][same]), (src, cf, k)
                n += int(same.sum())
            elif src.startswith("g9"):
                t = src[2:]
                for a, k in zip((h, v, d), ("hor", "ver", "dout")):
                    assert np.array_equal(a, g9["%s_%s_cf%d" % (t, k, cf)][dict(K.G9_SLICES)[t]]), (src, cf, k)
    assert n >= 450


def test_g10_sets_differ_from_the_defaults():
    """Every non-default set moves some split (the fixture can tell a kernel that ignores a threshold), and the probe triples
    split as probe_triples says: at float32(0.7) and above the gating picks the direction, just below it the error does - a double
    compare against 0.7 would treat float32(0.7) as "below"."""
    g10 = golden("g10_m2p_params.npz")
    for name in K.SETS:
        if name == "defaults":
            continue
        moved = 0
        for cf in (1, 2):
            for src, _, _, _ in K.inputs(cf, 0.5):
                if src == "probe":
                    continue
                a, b = K.expected(g10, name, src, cf), K.expected(g10, "defaults", src, cf)
                moved += int(sum(np.any(x != y, axis=tuple(range(1, x.ndim))) for x, y in zip(a, b)).astype(bool).sum())
        assert moved > 0, name
    for name in ("thd_0p7",):
        for cf in (1, 2):
            h, v, _ = K.expected(g10, name, "probe", cf)
            # nh = 140, values t, up, down, each with its mirror: H, V, H, V, V, H (mirror of "down" counts 116 vertical vs 0)
            kinds = ["H" if h[i, 8].all() else ("V" if v[i, :, 8].all() else "0") for i in range(6)]
            assert kinds == ["H", "V", "H", "V", "V", "H"], (name, cf, kinds)
