"""GPU: Map2Partition thresholds (include/pmp.h: pmp_partition_params) through every post-processing entry point, bit-exact with the
reference-made fixture G10 (tests/golden/g10_m2p_params.npz; inputs rebuilt by tests/m2p_params_cases.py), captured at enqueue
(asynchronous *_device calls, range-guard replays), per component, and through the CLI driver's --m2p / --m2pChroma."""
import os
import time

import numpy as np
import pytest

from conftest import golden
import gpu_rig
import m2p_params_cases as K
from oracle import parity as Y

pytestmark = pytest.mark.gpu

COMPS = {1: "Luma", 2: "Chroma"}

eng = gpu_rig.engine_fixture(synthetic_mtt=True)


@pytest.fixture
def e(eng):
    """The module's engine, its thresholds back at the defaults after the test."""
    yield eng
    eng.synchronize()
    for comp in COMPS.values():
        eng.set_partition_params(comp)


@pytest.fixture(scope="module")
def g10():
    return golden("g10_m2p_params.npz")


def stacked(cf, thd):
    """All inputs of one chroma factor in one batch + the per-source row ranges."""
    parts = K.inputs(cf, thd)
    rows, o = {}, 0
    for src, qt, _, _ in parts:
        rows[src] = slice(o, o + len(qt))
        o += len(qt)
    return tuple(np.concatenate([p[i] for p in parts]) for i in (1, 2, 3)) + (rows,)


def check_set(g10, name, cf, h, v, d, rows):
    for src, sl in rows.items():
        eh, ev, ed = K.expected(g10, name, src, cf)
        assert np.array_equal(h[sl], eh) and np.array_equal(v[sl], ev) and np.array_equal(d[sl], ed), (name, src, cf)


def test_postprocess_equals_reference_for_every_set(e, g10):
    """pmp_postprocess under every set of G10, both components: the reference's outputs bit for bit.  The fixture ran
    eli_structual_error first (as seq_post_process does), so every row compares, not only those the QT fix leaves alone."""
    n = 0
    for name, vals in K.SETS.items():
        for cf, comp in COMPS.items():
            e.set_partition_params(comp, **K.kw(name))
            got = e.get_partition_params(comp)
            assert [got[k] for k in ("lamb1", "lamb2", "lamb3", "lamb4", "lamb5")] == list(vals[:5])
            assert got["thd"] == float(np.float32(vals[5]))
            qt, bt, dire, rows = stacked(cf, vals[5])
            h, v, q8, d = e.post_process(qt, bt, dire, comp)
            check_set(g10, name, cf, h, v, d, rows)
            n += len(qt)
    # a non-default set over the value range the nets can emit (G3b: |logit| up to 3e38, +-inf, NaN), raw QT logits
    for cf, comp in COMPS.items():
        e.set_partition_params(comp, **K.kw(K.G3B_SET))
        qt, bt, dire, _ = K.g3b_inputs(cf)
        h, v, q8, d = e.post_process(qt, bt, dire, comp)
        eh, ev, ed = K.expected(g10, K.G3B_SET, "g3b", cf)
        assert np.array_equal(h, eh) and np.array_equal(v, ev) and np.array_equal(d, ed), cf
        assert np.array_equal(q8, golden("g3b_m2p_range.npz")["q8_cf%d" % cf][K.G3B_SLICE])
    assert n > 8 * 2 * 300


def test_null_restores_the_defaults_and_components_are_independent(e, g10):
    qt1, bt1, dire1, rows1 = stacked(1, 0.5)
    qt2, bt2, dire2, rows2 = stacked(2, 0.5)
    e.set_partition_params("Luma", **K.kw("early_stop"))
    e.set_partition_params("Chroma", **K.kw("ties"))
    h, v, _, d = e.post_process(qt1, bt1, dire1, "Luma")
    check_set(g10, "early_stop", 1, h, v, d, rows1)
    h, v, _, d = e.post_process(qt2, bt2, dire2, "Chroma")
    check_set(g10, "ties", 2, h, v, d, rows2)
    e.set_partition_params("Luma")                               # NULL: the reference's defaults, G3's outputs again
    from pmp_vvc_tip2023_amd import engine
    assert e.get_partition_params("Luma") == engine.DEFAULT_PARTITION_PARAMS
    assert e.get_partition_params("Chroma") == dict(zip(engine.PARAM_KEYS, K.SETS["ties"][:5] + (0.5,)))
    h, v, _, d = e.post_process(qt1, bt1, dire1, "Luma")
    check_set(g10, "defaults", 1, h, v, d, rows1)
    g = golden("g3_m2p.npz")
    sl = rows1["g3q"]
    assert np.array_equal(h[sl], g["q_hor_cf1"][K.G3_SLICES[0][1]]) and np.array_equal(d[sl], g["q_dout_cf1"][K.G3_SLICES[0][1]])
    h, v, _, d = e.post_process(qt2, bt2, dire2, "Chroma")       # chroma kept its own set
    check_set(g10, "ties", 2, h, v, d, rows2)


def test_rejected_sets_leave_the_old_one_in_force(e, g10):
    from pmp_vvc_tip2023_amd import _lib
    e.set_partition_params("Luma", **K.kw("ties"))
    before = e.get_partition_params("Luma")
    for bad in ({"lamb5": 0.5}, {"lamb5": 0.6699999999999999}, {"lamb1": float("nan")}, {"thd": 0.0}, {"thd": 2.5},
                {"lamb2": float("inf")}, {"lamb4": -0.1}, {"lamb1": 0.5, "lamb3": -1.0}):
        with pytest.raises(_lib.PmpError) as ei:
            e.set_partition_params("Luma", **bad)
        assert ei.value.code == -1
        assert e.get_partition_params("Luma") == before
    with pytest.raises(TypeError):
        e.set_partition_params("Luma", lamb6=0.5)
    qt, bt, dire, rows = stacked(1, 0.5)
    h, v, _, d = e.post_process(qt, bt, dire, "Luma")
    check_set(g10, "ties", 1, h, v, d, rows)


def test_seq_post_process_keywords(e, g10):
    """Engine.seq_post_process takes the reference's keyword names for one call and leaves the component's set as it was."""
    qt, bt, dire, rows = stacked(2, 1.5)
    n = len(qt)
    h, v, _, d = e.seq_post_process(qt, bt, dire, "Chroma", n, 64, 64, None, **K.kw("thd_1p5"))
    check_set(g10, "thd_1p5", 2, h, v, d, rows)
    from pmp_vvc_tip2023_amd import engine
    assert e.get_partition_params("Chroma") == engine.DEFAULT_PARTITION_PARAMS


def test_fused_and_record_entry_points_use_the_set(e):
    """pmp_infer_postprocess (host), pmp_infer_postprocess_device, pmp_infer_postprocess_records_device and
    pmp_postprocess_records_device under a non-default set equal pmp_postprocess on the fused call's own device logits."""
    import torch
    from pmp_vvc_tip2023_amd import parallel, synth
    y, u, v = synth.recipe_r_blocks(48, 17)
    dev = torch.device("cuda", 0)
    for comp, name in (("Luma", "early_stop"), ("Chroma", "permissive")):
        e.set_partition_params(comp, **K.kw(name))
        h, vv, q8, d8, qt, bt, dire = e.infer_postprocess(comp, 22, y, u, v, want_logits=True)
        ref = e.post_process(qt, bt, dire, comp)
        for a, b in zip((h, vv, q8, d8), ref):
            assert np.array_equal(a, b), comp
        ty, tu, tv = (torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (y, u, v))
        n = len(y)
        rec = torch.empty((n, parallel.RECORD), dtype=torch.uint8, device=dev)
        e.infer_postprocess_records_device(comp, 22, ty.data_ptr(), tu.data_ptr(), tv.data_ptr(), n, rec.data_ptr())
        dq = torch.empty((n, 64), device=dev); db = torch.empty((n, 768), device=dev); dd = torch.empty((n, 768), device=dev)
        o = [torch.empty((n, 256), dtype=torch.uint8, device=dev), torch.empty((n, 256), dtype=torch.uint8, device=dev),
             torch.empty((n, 64), dtype=torch.uint8, device=dev), torch.empty((n, 768), dtype=torch.int8, device=dev)]
        e.infer_postprocess_device(comp, 22, ty.data_ptr(), tu.data_ptr(), tv.data_ptr(), n, *(t.data_ptr() for t in o),
                                   dq.data_ptr(), db.data_ptr(), dd.data_ptr())
        rec2 = torch.empty_like(rec)
        e.postprocess_records_device(comp, dq.data_ptr(), db.data_ptr(), dd.data_ptr(), n, rec2.data_ptr())
        e.synchronize()
        own = e.post_process(dq.cpu().numpy(), db.cpu().numpy(), dd.cpu().numpy(), comp)   # the fused call's own device logits
        for got in (parallel.unpack_records(rec.cpu().numpy()), parallel.unpack_records(rec2.cpu().numpy()),
                    [t.cpu().numpy() for t in o]):
            for a, b in zip(got, own):
                assert np.array_equal(np.asarray(a).reshape(b.shape), b), comp


def test_device_calls_capture_the_set_at_enqueue(e, g10):
    """Two pmp_postprocess_device calls enqueued back to back with different sets, and the set changed again before anything was
    synchronised: each call has the outputs of its own set."""
    import torch
    dev = torch.device("cuda", 0)
    qt, bt, dire, rows = stacked(1, 0.5)
    n = len(qt)
    tq, tb, td = (torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (qt, bt, dire))
    outs = []
    for name in ("early_stop", "ties", "permissive"):
        e.set_partition_params("Luma", **K.kw(name))
        o = [torch.empty((n, 256), dtype=torch.uint8, device=dev), torch.empty((n, 256), dtype=torch.uint8, device=dev),
             torch.empty((n, 64), dtype=torch.uint8, device=dev), torch.empty((n, 768), dtype=torch.int8, device=dev)]
        e.postprocess_device("Luma", tq.data_ptr(), tb.data_ptr(), td.data_ptr(), n, *(t.data_ptr() for t in o))
        outs.append((name, o))
    e.set_partition_params("Luma", **K.kw("lamb3_0p8"))
    e.synchronize()
    for name, o in outs:
        h, v, _, d = (t.cpu().numpy() for t in o)
        check_set(g10, name, 1, h.reshape(n, 16, 16), v.reshape(n, 16, 16), d.reshape(n, 3, 16, 16), rows)


def test_range_guard_replay_uses_the_set_captured_at_enqueue(g10):
    """A saturated f16x3 inference call is re-run at pmp_synchronize and the post-processing enqueued behind it is replayed
    (include/pmp.h).  The set is changed between enqueue and pmp_synchronize: the replay still runs with the set of its enqueue."""
    import torch
    from pmp_vvc_tip2023_amd import engine
    dev = torch.device("cuda", 0)
    y = np.ascontiguousarray(golden("g1_qt.npz")["block_y"][:6])
    e2 = engine.Engine(0, allow_synthetic_mtt=True)
    try:
        e2.set_precision("f16x3")
        e2.load("Luma", 22)
        e2.load_pretrain_model("Luma_MSBD", 22, Y.range_stress_weights())
        e2.set_activation_scales(False)                  # activations leave the fp16 range: the guard fires (test_f16x3_range_guard)
        n = len(y)
        ty = torch.from_numpy(y).to(dev)
        dq = torch.empty((n, 64), device=dev); db = torch.empty((n, 768), device=dev); dd = torch.empty((n, 768), device=dev)
        o = [torch.empty((n, 256), dtype=torch.uint8, device=dev), torch.empty((n, 256), dtype=torch.uint8, device=dev),
             torch.empty((n, 64), dtype=torch.uint8, device=dev), torch.empty((n, 768), dtype=torch.int8, device=dev)]
        e2.set_partition_params("Luma", **K.kw("early_stop"))
        e2.infer_device("Luma", 22, ty.data_ptr(), None, None, n, dq.data_ptr(), db.data_ptr(), dd.data_ptr())
        e2.postprocess_device("Luma", dq.data_ptr(), db.data_ptr(), dd.data_ptr(), n, *(t.data_ptr() for t in o))
        e2.set_partition_params("Luma", **K.kw("thd_1p5"))          # changed before the flag is looked at
        e2.synchronize()
        assert e2.saturated() and e2.saturation_reruns() == 1
        lq, lb, ld = dq.cpu().numpy(), db.cpu().numpy(), dd.cpu().numpy()    # the re-run's (fp32) logits
        got = [t.cpu().numpy() for t in o]
        e2.set_partition_params("Luma", **K.kw("early_stop"))
        want = e2.post_process(lq, lb, ld, "Luma")
        for a, b in zip(got, want):
            assert np.array_equal(a.reshape(b.shape), b)
        e2.set_partition_params("Luma", **K.kw("thd_1p5"))
        other = e2.post_process(lq, lb, ld, "Luma")
        print("replay: outputs under the later set differ from the captured set's: %s"
              % any(not np.array_equal(a, b) for a, b in zip(want, other)))
    finally:
        e2.close()


def test_permissive_set_on_the_largest_trees_is_bounded(e, g10):
    """G3's largest candidate trees (6288 leaves for luma with the defaults) under the permissive set (lamb1 = 1, lamb5 = 0.67, the
    lowest lamb5 the domain admits): bounded time, bit-exact where G10 has them."""
    g = golden("g3_m2p.npz")
    for cf, comp in COMPS.items():
        qt = g["t_qt_cf%d" % cf].astype(np.float32); bt = g["t_bt_cf%d" % cf]; dire = g["t_dire_cf%d" % cf]
        e.set_partition_params(comp, **K.kw("permissive"))
        e.post_process(qt[:1], bt[:1], dire[:1], comp)                   # warm-up
        t0 = time.perf_counter()
        h, v, _, d = e.post_process(qt, bt, dire, comp)
        dt = time.perf_counter() - t0
        e.set_partition_params(comp)
        t0 = time.perf_counter()
        e.post_process(qt, bt, dire, comp)
        dt0 = time.perf_counter() - t0
        print("largest trees, %s: %d blocks in %.4f s under the permissive set, %.4f s with the defaults" % (comp, len(qt), dt, dt0))
        assert dt < 5.0
        sl = dict(K.G3_SLICES)["t"]
        eh, ev, ed = K.expected(g10, "permissive", "g3t", cf)
        assert np.array_equal(h[sl], eh) and np.array_equal(v[sl], ev) and np.array_equal(d[sl], ed)


def _sequence(tmp_path):
    from pmp_vvc_tip2023_amd import synth
    inp = tmp_path / "in"; cfg = tmp_path / "cfg"
    inp.mkdir(); cfg.mkdir()
    w, h, fr = 256, 192, 2
    with open(inp / "table.txt", "w") as f:
        f.write("SeqM,SeqM_256x192_30.yuv,%d,%d,%d,30\n#end!!!!\n" % (w, h, fr))
    y, u, v = synth.recipe_r_frames(fr, h, w, 23)
    with open(inp / "SeqM_256x192_30.yuv", "wb") as f:
        for i in range(fr):
            f.write(y[i].tobytes()); f.write(u[i].tobytes()); f.write(v[i].tobytes())
    with open(cfg / "SeqM.cfg", "w") as f:
        f.write("InputFile                     : SeqM_256x192_30.yuv\nInputBitDepth                 : 8\n")
    return inp, cfg, (y, u, v), (fr, h, w)


def test_driver_m2p_flags(e, tmp_path, capfd):
    """--m2p / --m2pChroma: the files equal the formatted records under those sets; the defaults spelled out give the bytes of no flag."""
    from pmp_vvc_tip2023_amd import engine as E, inference_qbd as D
    inp, cfg, (y, u, v), (fr, h, w) = _sequence(tmp_path)

    def run(tag, extra):
        out = tmp_path / ("out_" + tag)
        D.main(["--jobID", "m", "--inputDir", str(inp), "--outDir", str(out), "--seqTable", "table.txt", "--cfgDir", str(cfg), "--ssRatio", "1",
                "--startSeqID", "0", "--seqNum", "1", "--qps", "22", "--allowSyntheticMTT"] + extra)
        d = out / "m" / "PartitionMat"
        return {n: open(d / n, "rb").read() for n in sorted(os.listdir(d))}

    spec_l = ",".join("%s=%r" % kv for kv in K.kw("early_stop").items())
    spec_c = "lamb5=0.9,thd=0.7"
    capfd.readouterr()
    got = run("m2p", ["--m2p", spec_l, "--m2pChroma", spec_c])
    err = capfd.readouterr().err
    assert err.count("Map2Partition thresholds (Luma)") == 1 and err.count("Map2Partition thresholds (Chroma)") == 1
    plain = run("none", [])
    assert "Map2Partition thresholds" not in capfd.readouterr().err
    spelled = run("spelled", ["--m2p", "lamb1=0.7,lamb2=0.7,lamb3=1.5,lamb4=0.3,lamb5=0.7,thd=0.5", "--m2pChroma", "thd=0.5"])
    assert list(plain) == list(spelled) == list(got) and len(got) == 2
    for n in plain:
        assert plain[n] == spelled[n], n
    by, bu, bv = e.output_block_yuv(y, u, v, 8)
    sets = {"Luma": E.parse_partition_params(spec_l), "Chroma": E.parse_partition_params(spec_c, E.parse_partition_params(spec_l))}
    for comp, prm in sets.items():
        e.set_partition_params(comp, **prm)
        hh, vv, q8, d8 = e.infer_postprocess(comp, 22, by, bu, bv)
        name = [n for n in got if "_%s_" % comp in n][0]
        assert got[name] == E.format_partition_text(fr, h, w, hh, vv, q8, d8), comp
        e.set_partition_params(comp)
        hh, vv, q8, d8 = e.infer_postprocess(comp, 22, by, bu, bv)
        assert plain[name] == E.format_partition_text(fr, h, w, hh, vv, q8, d8), comp
