"""GPU parity tests: the HIP path through the C ABI against (a) golden vectors made by the imported reference and
(b) the pinned oracle on the same seeded inputs.  Logits: 1e-3 absolute (north_star); integers: bit-exact."""
import numpy as np
import pytest
import torch

import gpu_rig
from conftest import g3_sets, g3b_sets, golden, golden_path
from oracle import parity as Y

pytestmark = pytest.mark.gpu
TOL = 1e-3  # north_star: "within 1e-3 fp32 on the map logits"

# every parity test runs on all three convolution datapaths (fp16 2-term split, bf16 3-term split, exact fp32 MFMA)
eng = gpu_rig.engine_fixture(gpu_rig.DATAPATHS, synthetic_mtt=True)


@pytest.fixture(scope="module")
def g1():
    return golden("g1_qt.npz")


# ------------------------------------------------------------------------------------------------ nets
@pytest.mark.parametrize("comp", ["Luma", "Chroma"])
@pytest.mark.parametrize("qp", [22, 27, 32, 37])
def test_qt_and_mtt_logits_vs_reference_golden(eng, g1, comp, qp):
    """G1 (real QT weights) and G2 (synthetic MTT weights) through pmp_infer."""
    g2 = golden("g2_msbd.npz")
    qt, bt, dire = eng.inference_pre_QBD(comp, qp, g1["block_y"], g1["block_u"], g1["block_v"])
    assert eng.provenance[(comp + "_Q", qp)].endswith(".pmpw")
    assert qt.shape == (16, 1, 8, 8) and bt.shape == (16, 3, 16, 16)
    eq = np.abs(qt - g1["qt_%s_%d" % (comp, qp)]).max()
    assert eq < TOL, "QT logits off by %g" % eq
    for k in range(3):
        ref = g2["out%d_%s_%d" % (k, comp, qp)]           # [8,2,16,16] reference heads (ch0 depth, ch1 direction)
        eb = np.abs(bt[:8, k] - ref[:, 0]).max()
        ed = np.abs(dire[:8, k] - ref[:, 1]).max()
        assert eb < TOL and ed < TOL, "MTT layer %d off by %g / %g" % (k, eb, ed)


def test_config1_single_block_plumbing(eng, g1):
    """BASELINE.json configs[0]: Luma QT-net QP22 on a single block."""
    qt, _, _ = eng.inference_pre_QBD("Luma", 22, g1["block_y"][:1])
    assert np.abs(qt - g1["qt_Luma_22"][:1]).max() < TOL


@pytest.mark.parametrize("comp", ["Luma", "Chroma"])
def test_logits_vs_oracle_fresh_inputs_and_chunking(eng, comp):
    """Fresh seeded blocks: HIP vs the torch oracle; ragged chunking (chunk=5 over 13 blocks) is bit-identical
    to one pass; extreme inputs (all 0, all 255) included."""
    from pmp_vvc_tip2023_amd import synth
    y, u, v = synth.recipe_r_blocks(13, 101)
    Y.extreme_blocks(y, u, v, count=2)
    qp = 27
    qt, bt, dire = eng.inference_pre_QBD(comp, qp, y, u, v)
    oq, obt, odire = Y.oracle_logits(comp, qp, y, u, v)
    assert np.abs(qt - oq).max() < TOL and np.abs(bt - obt).max() < TOL and np.abs(dire - odire).max() < TOL
    eng.set_chunk(5)
    try:
        qt2, bt2, dire2 = eng.inference_pre_QBD(comp, qp, y, u, v)
    finally:
        eng.set_chunk(4096)
    assert np.array_equal(qt, qt2) and np.array_equal(bt, bt2) and np.array_equal(dire, dire2)


def _oracle_512(comp, qp):
    """Oracle logits and end-to-end flags of 512 fresh recipe-R blocks (computed once, shared by the three datapaths and with
    tests/test_gpu_val_stats.py, which asks for the same blocks)."""
    return Y.fresh_oracle(comp, qp, 512, 1000 + qp + (7 if comp == "Chroma" else 0), flags=True)


@pytest.mark.parametrize("comp", ["Luma", "Chroma"])
@pytest.mark.parametrize("qp", [22, 27, 32, 37])
def test_512_fresh_blocks_logits_and_end_to_end_flags_vs_oracle(eng, comp, qp):
    """SURVEY 8(d) at a size that means something: 512 fresh blocks per component and QP.  Logits within 1e-3 of the torch oracle;
    split flags of the HIP path (its own logits) against the oracle's end-to-end flags (its own logits).  'Bit-exact flags' is
    only defined for identical logits: a value that sits within the logit difference of a rounding boundary
    may legitimately land on the other side, so the audit counts those cells and allows mismatches only in blocks that have one."""
    y, u, v, oq, obt, odire, oflags = _oracle_512(comp, qp)
    hor, ver, q8, d8, qt, bt, dire = eng.infer_postprocess(comp, qp, y, u, v, want_logits=True)
    err = Y.per_block_error((qt, bt, dire), (oq, obt, odire)).max()
    assert err < TOL, "%s QP%d logits off by %g" % (comp, qp, err)
    margin = max(2e-4, 2 * float(err))
    bad, risky = Y.boundary_audit(oq, obt, odire, (hor, ver, q8, d8), oflags, margin)
    assert not (bad & ~risky).any(), "%d blocks differ from the oracle's flags without a value near a rounding boundary" % int((bad & ~risky).sum())
    assert bad.sum() <= 8, "%d of 512 blocks differ (near-boundary blocks: %d)" % (int(bad.sum()), int(risky.sum()))


@pytest.mark.parametrize("shape", [(8, 32, 32, 48, 64, 3), (8, 32, 32, 16, 64, 3), (4, 16, 16, 80, 64, 5), (8, 16, 16, 96, 32, 3),
                                   (4, 16, 16, 48, 16, 3), (8, 32, 32, 32, 64, 1), (4, 48, 32, 64, 64, 3)])
def test_conv_kernel_shapes_beyond_the_nets(eng, shape):
    """Convolution shapes the four nets never launch (odd channel-group counts: the unpaired K order of the split kernels;
    1x1; non-square maps): the split datapaths against the exact fp32 MFMA kernel on the same random tensors
    (pmp_debug_conv_bench, include/pmp.h).  A context on the fp32 datapath compares against the bf16x6 kernel (include/pmp.h): there
    the comparison must hold too, and give exactly the numbers of a bf16x6 context (both kernels are deterministic, the tensors seeded)."""
    import ctypes as C
    n, h, w, ci, co, k = shape

    def bench():
        a, b, d, r = C.c_double(), C.c_double(), C.c_double(), C.c_double()
        eng._ck(eng.lib.pmp_debug_conv_bench(eng.h, n, h, w, ci, co, k, 1, C.byref(a), C.byref(b), C.byref(d), C.byref(r)))
        return d.value, r.value
    d, r = bench()
    assert r > 0.5 and d < 1e-4 * max(1.0, r), (shape, d, r)
    if eng.get_precision() == "fp32":
        eng.set_precision("bf16x6")
        try:
            assert bench() == (d, r), shape
        finally:
            eng.set_precision("fp32")


def test_small_calls_need_small_workspaces():
    """The activation arena is sized for the blocks a pass runs, not for the chunk (include/pmp.h): a 4-block call stays in the
    tens of megabytes, so several contexts (or a co-tenant) fit beside each other on one GPU."""
    from pmp_vvc_tip2023_amd import engine, synth
    e2 = engine.Engine(0, allow_synthetic_mtt=True)
    try:
        assert e2.workspace_bytes() == 0
        y, u, v = synth.recipe_r_blocks(4, 3)
        e2.infer_postprocess("Luma", 22, y)
        assert 0 < e2.workspace_bytes() <= 4 * 2.75 * 2 ** 20
        e2.infer_postprocess("Chroma", 22, y, u, v)
        e2.set_precision("bf16x6")
        e2.infer_postprocess("Luma", 22, y)
        assert e2.workspace_bytes() <= 4 * 4.1 * 2 ** 20
    finally:
        e2.close()


def test_parked_workspace_is_reused_and_trimmed(g1):
    """pmp_destroy parks a large activation workspace for the next context on the device (a 10 GB hipMalloc right after a hipFree
    stalls 0.5-1.4 s now and then on this hardware, profiles/r03_notes.txt); pmp_trim gives it back.  Results do not depend on where
    the workspace came from, and a context reports what its passes NEED, not the size of a buffer it took over."""
    from pmp_vvc_tip2023_amd import engine
    y = np.concatenate([g1["block_y"]] * 8)                  # 128 luma blocks: 320 MB of workspace, above the parking threshold
    outs, need = [], []
    for k in range(3):
        e2 = engine.Engine(0, allow_synthetic_mtt=True)
        try:
            outs.append(e2.inference_pre_QBD("Luma", 22, y if k != 1 else y[:64]))
            need.append(e2.workspace_bytes())
        finally:
            e2.close()
        if k == 1:
            assert e2.lib.pmp_trim() == 0                    # the third context allocates afresh
    assert need[0] == need[2] and 0 < need[1] < need[0]      # the second context ran in the first one's (larger) buffer
    for a, b in zip(outs[0], outs[2]):
        assert np.array_equal(a, b)
    for a, b in zip(outs[0], outs[1]):
        assert np.array_equal(a[:64], b)
    assert e2.lib.pmp_trim() == 0


def test_parking_can_be_turned_off(g1, monkeypatch):
    """PMP_PARK_WORKSPACE=0: pmp_destroy returns the whole workspace to the driver (a host that hands the VRAM to another library and
    cannot call pmp_trim); by default the 320 MB of this pass stay parked until pmp_trim."""
    import torch
    from pmp_vvc_tip2023_amd import engine
    y = np.concatenate([g1["block_y"]] * 8)

    def held_after_destroy():
        e2 = engine.Engine(0, allow_synthetic_mtt=True)
        e2.lib.pmp_trim()
        torch.cuda.synchronize(0)
        before = torch.cuda.mem_get_info(0)[0]
        try:
            e2.inference_pre_QBD("Luma", 22, y)
        finally:
            e2.close()
        return before - torch.cuda.mem_get_info(0)[0], e2.lib

    held, lib = held_after_destroy()
    assert held > 200 * 2 ** 20
    assert lib.pmp_trim() == 0
    monkeypatch.setenv("PMP_PARK_WORKSPACE", "0")
    held, lib = held_after_destroy()
    assert held < 64 * 2 ** 20
    assert lib.pmp_trim() == 0


def test_overlap_mode_is_bit_identical(g1):
    """pmp_set_overlap: a call of >= 1024 blocks runs as two chunks on two streams with two workspaces.  Logits and flags equal the
    default mode's bit for bit (both components, a ragged size, records through the device entry point), smaller calls are not cut, and
    a range-guard re-run behind an overlapped call still repairs it."""
    import torch
    from pmp_vvc_tip2023_amd import engine, synth, weights as W
    n = 1500
    y, u, v = synth.recipe_r_blocks(n, 21)
    e = engine.Engine(0, allow_synthetic_mtt=True)
    try:
        for comp in ("Luma", "Chroma"):
            ref = e.infer_postprocess(comp, 22, y, u, v, want_logits=True)
            need = e.workspace_bytes()
            e.set_overlap(True)
            got = e.infer_postprocess(comp, 22, y, u, v, want_logits=True)
            assert need < e.workspace_bytes() <= 2 * need         # + the second workspace, sized for a half-call chunk, while the mode is on
            small = e.infer_postprocess(comp, 22, y[:700], u[:700], v[:700], want_logits=True)     # below the threshold: one chunk
            e.set_overlap(False)
            assert e.workspace_bytes() == need                    # turning the mode off frees the second workspace
            for a, b in zip(ref, got):
                assert np.array_equal(a, b), comp
            for a, b in zip(ref, small):
                assert np.array_equal(a[:700], b), comp
        # records through the device-pointer entry point, twice in flight
        dev = torch.device("cuda:0")
        d_y = torch.from_numpy(y).to(dev)
        recs = []
        for ov in (False, True):
            e.set_overlap(ov)
            r = [torch.empty((n, 1344), dtype=torch.uint8, device=dev) for _ in range(2)]
            for k in range(2):
                e.infer_postprocess_records_device("Luma", 22, d_y.data_ptr(), None, None, n, r[k].data_ptr())
            e.synchronize()
            recs.append([x.cpu().numpy() for x in r])
        assert all(np.array_equal(recs[0][0], x) for x in recs[0][1:] + recs[1])
        # the range guard under overlap: stress weights saturate f16x3 in every chunk; the call is re-run on fp32 MFMA as a whole
        w = Y.range_stress_weights()
        yy = np.ascontiguousarray(np.concatenate([g1["block_y"]] * 70)[:1100])
        e.load("Luma", 22)
        e.load_pretrain_model("Luma_MSBD", 22, w)
        e.set_activation_scales(False)                           # with the calibrated scales these weights stay inside fp16 (test_f16x3_range_guard)
        e.set_overlap(False)
        q0, b0, d0 = e.inference_pre_QBD("Luma", 22, yy)
        r0 = e.saturation_reruns()
        e.set_overlap(True)
        q1, b1, d1 = e.inference_pre_QBD("Luma", 22, yy)
        assert e.saturation_reruns() == r0 + 1 and r0 >= 1
        assert np.array_equal(q0, q1) and np.array_equal(b0, b1) and np.array_equal(d0, d1)
    finally:
        e.close()


def test_default_chunk_boundary(eng):
    """More blocks than one library pass (default chunk 4096): the ragged second pass gives what a call on those blocks alone gives."""
    from pmp_vvc_tip2023_amd import synth
    y, _, _ = synth.recipe_r_blocks(16, 11)
    big = np.concatenate([y] * 257)[:4100]                    # 4096 + 4
    qt, bt, dire = eng.inference_pre_QBD("Luma", 22, big)
    q2, b2, d2 = eng.inference_pre_QBD("Luma", 22, big[4096:])
    assert np.array_equal(qt[4096:], q2) and np.array_equal(bt[4096:], b2) and np.array_equal(dire[4096:], d2)
    q3, b3, d3 = eng.inference_pre_QBD("Luma", 22, big[:16])
    assert np.array_equal(qt[:16], q3) and np.array_equal(bt[:16], b3) and np.array_equal(dire[:16], d3)


def test_caller_supplied_weights_and_errors(eng, g1):
    from pmp_vvc_tip2023_amd import _lib, engine, synth
    e2 = engine.Engine(0, allow_synthetic_mtt=True)
    try:
        with pytest.raises(_lib.PmpError) as ei:           # nothing loaded yet
            e2._ck(e2.lib.pmp_infer(e2.h, 0, 22, None, None, None, 1, None, None, None))
        assert ei.value.code == -1
        w = synth.synth_msbd_weights("Luma", 22)
        bad = dict(w); bad.pop("conv_B3.bias")
        with pytest.raises(_lib.PmpError) as ei:
            e2.load_pretrain_model("Luma_MSBD", 22, bad)
        assert ei.value.code == -1 and "conv_B3.bias" in str(ei.value)
        bad = dict(w); bad["trunk_M1.0.left.0.weight"] = np.zeros((64, 32, 3, 3), np.float32)
        with pytest.raises(_lib.PmpError):
            e2.load_pretrain_model("Luma_MSBD", 22, bad)
        y = np.ascontiguousarray(g1["block_y"][:2])
        qt = np.zeros((2, 64), np.float32); bt = np.zeros((2, 768), np.float32); dr = np.zeros((2, 768), np.float32)
        rc = e2.lib.pmp_infer(e2.h, 0, 22, y.ctypes.data, None, None, 2, qt.ctypes.data, bt.ctypes.data, dr.ctypes.data)
        assert rc == -3                                     # PMP_E_NOWEIGHTS
        with pytest.raises(ValueError):
            e2.inference_pre_QBD("Chroma", 22, y)           # chroma without u/v
        # empty input
        q0, b0, d0 = eng.inference_pre_QBD("Luma", 22, y[:0])
        assert q0.shape == (0, 1, 8, 8) and b0.shape == (0, 3, 16, 16)
    finally:
        e2.close()


def test_f16x3_range_guard(g1):
    """f16x3 carries activations as two fp16 terms, so values beyond +-65504 would be clamped (include/pmp.h).  The guard must
    (i) notice it, (ii) under the default policy return logits that are RIGHT (within 1e-3 of the oracle, by re-running the call
    on the exact fp32 MFMA datapath - which on the full-size campaign is the datapath closest to the oracle, 1.8x inside the tolerance
    on its worst block where bf16x6 is 1.1x), (iii) return PMP_E_RANGE under PMP_SAT_ERROR, and (iv) under PMP_SAT_IGNORE still never produce inf/NaN."""
    from pmp_vvc_tip2023_amd import _lib, engine
    y = np.ascontiguousarray(g1["block_y"][:6])
    w = Y.range_stress_weights()
    oq, obt, odire = want = Y.oracle_logits("Luma", 22, y, wbd=w)
    assert np.abs(obt).max() < 50                             # the logits themselves are ordinary
    e2 = engine.Engine(0, allow_synthetic_mtt=True)
    try:
        e2.set_precision("f16x3")
        e2.load("Luma", 22)                                    # real QT net; MTT net replaced below
        assert not e2.saturated() and e2.saturation_reruns() == 0
        e2.load_pretrain_model("Luma_MSBD", 22, w)
        # (o) round 5: with the activation scales the calibration pass chooses (include/pmp.h) these weights - a power-of-two stress - no longer
        # leave the fp16 range at all: right logits on the default datapath, no flag, no re-run
        qs, bs, ds = e2.inference_pre_QBD("Luma", 22, y)
        assert not e2.saturated() and e2.saturation_reruns() == 0
        assert Y.per_block_error((qs, bs, ds), want).max() < TOL
        assert e2.activation_report("Luma", 22)["exps"][0] >= 5           # trunk activations of 2e5..5e5 against the 4096 target
        e2.set_activation_scales(False)                         # the guard itself, from here on: exponents of zero
        qt, bt, dire = e2.inference_pre_QBD("Luma", 22, y)     # default policy: re-run on fp32 MFMA
        assert e2.saturated() and e2.saturation_reruns() == 1
        err = Y.per_block_error((qt, bt, dire), want).max()
        assert err < TOL, "range guard re-run is off by %g" % err
        e2.set_precision("fp32")                               # the re-run IS the fp32 datapath: same bits
        qf, bf, df = e2.inference_pre_QBD("Luma", 22, y)
        assert np.array_equal(qf, qt) and np.array_equal(bf, bt) and np.array_equal(df, dire), "the guard's re-run is not the fp32 datapath"
        e2.set_precision("f16x3")
        hor, ver, q8, d8, qt2, bt2, dire2 = e2.infer_postprocess("Luma", 22, y, want_logits=True)   # the fused entry point too
        assert e2.saturation_reruns() == 2 and np.array_equal(bt2, bt) and np.array_equal(dire2, dire)
        e2.set_saturation_policy("error")
        with pytest.raises(_lib.PmpError) as ei:
            e2.inference_pre_QBD("Luma", 22, y)
        assert ei.value.code == -7
        e2.set_saturation_policy("ignore")
        e2.clear_saturation()
        assert not e2.saturated()
        q3, b3, d3 = e2.inference_pre_QBD("Luma", 22, y)
        assert np.isfinite(q3).all() and np.isfinite(b3).all() and np.isfinite(d3).all()
        assert e2.saturated()                                  # polled: the device word was raised
        assert max(np.abs(b3 - obt).max(), np.abs(d3 - odire).max()) > TOL   # ... and clamped activations do change the logits
        # the same weights on the other two datapaths need no guard
        for prec in ("bf16x6", "fp32"):
            e2.set_precision(prec)
            e2.clear_saturation()
            q4, b4, d4 = e2.inference_pre_QBD("Luma", 22, y)
            assert Y.per_block_error((q4, b4, d4), want).max() < TOL
            assert not e2.saturated()
    finally:
        e2.close()


def test_device_calls_do_not_stall_the_host_and_the_guard_still_repairs(g1, oracle_lib):
    """The *_device entry points stay asynchronous under the default range-guard policy (include/pmp.h): each call snapshots the
    flag behind its passes and returns; the snapshot is looked at by a later call / pmp_synchronize, which re-runs a saturated
    call on the fp32 MFMA datapath and replays the post-processing enqueued behind it.
      (i) two device calls back to back return to the host in a fraction of the time the GPU needs for them (event timestamps);
      (ii) call A on range-stress weights (saturates) followed at once by call B on ordinary weights: after ONE pmp_synchronize
           both have oracle-correct logits and flags, exactly one re-run was counted;
      (iii) a caller that chains pmp_infer_device -> pmp_postprocess_device gets its post-processing replayed too."""
    import time
    from pmp_vvc_tip2023_amd import engine, synth
    dev = torch.device("cuda:0")
    e2 = engine.Engine(0, allow_synthetic_mtt=True)
    try:
        e2.set_precision("f16x3")
        e2.set_activation_scales(False)                           # the stress weights below must saturate: exponents of zero (include/pmp.h)
        e2.load("Luma", 22)
        e2.load("Luma", 27)
        # ---- (i) no host stall
        n = 2048
        y, _, _ = synth.recipe_r_blocks(n, 77)
        d_y = torch.from_numpy(y).to(dev)
        rec = [torch.empty((n, 1344), dtype=torch.uint8, device=dev) for _ in range(2)]
        e2.infer_postprocess_records_device("Luma", 22, d_y.data_ptr(), None, None, n, rec[0].data_ptr())   # warm-up: workspace, code objects
        e2.infer_postprocess_records_device("Luma", 27, d_y.data_ptr(), None, None, n, rec[1].data_ptr())   # (a net's FIRST use packs its weights - and, with the
        e2.synchronize()                                                                                     #  activation scales on, calibrates: one host sync per net, include/pmp.h)
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        e2.infer_postprocess_records_device("Luma", 22, d_y.data_ptr(), None, None, n, rec[0].data_ptr())
        e2.infer_postprocess_records_device("Luma", 27, d_y.data_ptr(), None, None, n, rec[1].data_ptr())
        t_host = time.perf_counter() - t0
        e2.synchronize()
        t_all = time.perf_counter() - t0
        assert e2.saturation_reruns() == 0
        assert t_all > 0.04, "2 x 2048 luma blocks cannot finish in %.1f ms" % (t_all * 1e3)
        assert t_host < 0.5 * t_all, "two device calls held the host for %.1f ms of %.1f ms" % (t_host * 1e3, t_all * 1e3)
        # ---- (ii) a saturating call and an ordinary one in flight together
        yb = np.ascontiguousarray(g1["block_y"][:6])
        w_stress = Y.range_stress_weights()
        e2.load_pretrain_model("Luma_MSBD", 22, w_stress)
        oa = Y.oracle_logits("Luma", 22, yb, wbd=w_stress)
        ob = Y.oracle_logits("Luma", 27, yb)
        d_yb = torch.from_numpy(yb).to(dev)

        def outs():
            return (torch.zeros((6, 256), dtype=torch.uint8, device=dev), torch.zeros((6, 256), dtype=torch.uint8, device=dev),
                    torch.zeros((6, 64), dtype=torch.uint8, device=dev), torch.zeros((6, 768), dtype=torch.int8, device=dev),
                    torch.zeros((6, 64), device=dev), torch.zeros((6, 768), device=dev), torch.zeros((6, 768), device=dev))
        A, B = outs(), outs()
        e2.infer_postprocess_device("Luma", 22, d_yb.data_ptr(), None, None, 6, *[t.data_ptr() for t in A])
        e2.infer_postprocess_device("Luma", 27, d_yb.data_ptr(), None, None, 6, *[t.data_ptr() for t in B])
        e2.synchronize()
        assert e2.saturation_reruns() == 1 and e2.saturated()
        for got, want, qp in ((A, oa, 22), (B, ob, 27)):
            hor, ver, q8, d8 = (t.cpu().numpy() for t in got[:4])
            logits = [t.cpu().numpy().reshape(w.shape) for t, w in zip(got[4:], want)]
            err = Y.per_block_error(logits, want).max()
            assert err < TOL, "QP%d logits off by %g after the deferred re-run" % (qp, err)
            oflags = oh, ov, oq8, od8 = Y.oracle_flags("Luma", *logits)
            assert Y.flags_equal((hor.reshape(oh.shape), ver.reshape(ov.shape), q8.reshape(oq8.shape), d8.reshape(od8.shape)), oflags)
        # ---- (iii) separate infer + post-process calls: the post-processing behind a saturated call is replayed
        e2.clear_saturation()
        Cc = outs()
        e2.infer_device("Luma", 22, d_yb.data_ptr(), None, None, 6, Cc[4].data_ptr(), Cc[5].data_ptr(), Cc[6].data_ptr())
        e2.postprocess_device("Luma", Cc[4].data_ptr(), Cc[5].data_ptr(), Cc[6].data_ptr(), 6, Cc[0].data_ptr(), Cc[1].data_ptr(),
                              Cc[2].data_ptr(), Cc[3].data_ptr())
        e2.synchronize()
        assert e2.saturation_reruns() == 1
        for a, b in zip(A, Cc):
            assert torch.equal(a, b)
        # ---- (iv) both calls keep their logits in the CONTEXT's buffers (the record entry point passes no logit pointers): the re-run of A
        #      overwrites them, so B - ordinary weights, flag down - has to be run again before its post-processing is replayed; and a B
        #      with more blocks than A regrows those buffers, which must not happen under A's pending re-run.
        for nb in (6, 2100):                                      # 2100 > the 2048 blocks of (i): B regrows the context's logit buffers
            yb2, _, _ = synth.recipe_r_blocks(nb, 501)
            yb2[:6] = yb
            d_yb2 = torch.from_numpy(yb2).to(dev)
            e2.clear_saturation()
            ra = torch.zeros((6, 1344), dtype=torch.uint8, device=dev)
            rb = torch.zeros((nb, 1344), dtype=torch.uint8, device=dev)
            e2.infer_postprocess_records_device("Luma", 22, d_yb.data_ptr(), None, None, 6, ra.data_ptr())
            e2.infer_postprocess_records_device("Luma", 27, d_yb2.data_ptr(), None, None, nb, rb.data_ptr())
            e2.synchronize()
            assert e2.saturation_reruns() == 1
            # each call on its own: the reference for the pair in flight
            e2.clear_saturation()
            want_a = torch.empty((6, 1344), dtype=torch.uint8, device=dev)
            want_b = torch.empty((nb, 1344), dtype=torch.uint8, device=dev)
            e2.infer_postprocess_records_device("Luma", 22, d_yb.data_ptr(), None, None, 6, want_a.data_ptr())
            e2.synchronize()
            e2.infer_postprocess_records_device("Luma", 27, d_yb2.data_ptr(), None, None, nb, want_b.data_ptr())
            e2.synchronize()
            assert e2.saturation_reruns() == 1
            for a4, w4 in zip(A[:4], (want_a[:, :256], want_a[:, 256:512], want_a[:, 512:576], want_a[:, 576:].view(torch.int8))):
                assert torch.equal(a4, w4)                         # the record fields are the four arrays of (ii)
            assert torch.equal(ra, want_a), "records of the saturating call A differ after the deferred re-run (%d blocks in B)" % nb
            assert torch.equal(rb, want_b), "records of the ordinary call B were overwritten by A's re-run (%d blocks in B)" % nb
        # ---- (v) a saturating records call still pending when a HOST-pointer call arrives: the host call stages through the context's
        #      own logit buffers, which A's re-run writes - A must be settled first, and the host call must return ITS OWN results
        yh, _, _ = synth.recipe_r_blocks(9, 502)
        ref_h = e2.inference_pre_QBD("Luma", 27, yh)              # nothing pending: the reference
        ref_p = e2.post_process(*ref_h, "Luma")
        for host_call in ("infer", "postprocess", "infer_postprocess"):
            e2.clear_saturation()
            ra = torch.zeros((6, 1344), dtype=torch.uint8, device=dev)
            e2.infer_postprocess_records_device("Luma", 22, d_yb.data_ptr(), None, None, 6, ra.data_ptr())
            if host_call == "infer":
                got = e2.inference_pre_QBD("Luma", 27, yh)
                for a5, b5 in zip(got, ref_h):
                    assert np.array_equal(a5, b5), "pmp_infer behind a pending saturated call returned foreign logits"
            elif host_call == "postprocess":
                got = e2.post_process(*ref_h, "Luma")
                for a5, b5 in zip(got, ref_p):
                    assert np.array_equal(a5, b5), "pmp_postprocess behind a pending saturated call read foreign logits"
            else:
                got = e2.infer_postprocess("Luma", 27, yh, want_logits=True)
                for a5, b5 in zip(got, tuple(ref_p) + tuple(ref_h)):
                    assert np.array_equal(a5, b5), "pmp_infer_postprocess behind a pending saturated call returned foreign results"
            e2.synchronize()
            assert e2.saturation_reruns() == 1
            assert torch.equal(ra, want_a), "records of the saturating call A differ after a host call settled it (%s)" % host_call
        # ---- the error policy reports at the call that looks at the flag
        from pmp_vvc_tip2023_amd import _lib
        e2.set_saturation_policy("error")
        e2.infer_device("Luma", 22, d_yb.data_ptr(), None, None, 6, Cc[4].data_ptr(), Cc[5].data_ptr(), Cc[6].data_ptr())
        with pytest.raises(_lib.PmpError) as ei:
            e2.synchronize()
        assert ei.value.code == -7
        e2.synchronize()                                      # the context is usable again
    finally:
        e2.close()


@pytest.mark.parametrize("comp", ["Luma", "Chroma"])
def test_fused_16x16_tails_are_bit_identical(comp):
    """chain16.hip: on the f16x3 datapath the 16x16-resolution tails of the nets (MTT: trunk_B1/B2 + heads + attention 1; QT: resblock_q3 ..
    conv_q2) run as one launch per net with the activations in LDS.  Same weight streams, same K-step order, same epilogue arithmetic:
    the logits must equal the launch-per-layer path's BIT FOR BIT - on the golden blocks, on fresh ones (all-0 and all-255 included), at
    every QP, with a ragged chunk, and through the range guard's flag (the fused kernels raise it like the layer kernels do)."""
    from pmp_vvc_tip2023_amd import engine, synth
    g1 = golden("g1_qt.npz")
    y, u, v = synth.recipe_r_blocks(150, 4242)
    Y.extreme_blocks(y, u, v, count=2)
    y[2:18] = g1["block_y"]; u[2:18] = g1["block_u"]; v[2:18] = g1["block_v"]
    e = engine.Engine(0, allow_synthetic_mtt=True)
    try:
        e.set_precision("f16x3")
        for qp in (22, 27, 32, 37):
            e.set_fusion(True)
            a = e.inference_pre_QBD(comp, qp, y, u, v)
            e.set_fusion(False)
            b = e.inference_pre_QBD(comp, qp, y, u, v)
            for nm, p, q in zip(("qt", "bt", "dire"), a, b):
                assert np.array_equal(p, q), "%s QP%d %s: fused and per-layer paths differ by %g" % (comp, qp, nm, np.abs(p - q).max())
            assert np.isfinite(a[0]).all() and np.abs(a[1]).max() > 0.1      # not a comparison of two empty results
            for mode in (2, 3):      # each family of fused kernels alone: the 16x16 tails (chain16.hip), the 32x32 ResidualBlocks (rbfuse32.hip)
                e.set_fusion(mode)
                m = e.inference_pre_QBD(comp, qp, y, u, v)
                for nm, p, q in zip(("qt", "bt", "dire"), m, b):
                    assert np.array_equal(p, q), "%s QP%d %s: fusion mode %d and the per-layer path differ by %g" % (comp, qp, nm, mode, np.abs(p - q).max())
        e.set_fusion(True)
        e.set_chunk(37)
        try:
            c = e.inference_pre_QBD(comp, 37, y, u, v)
        finally:
            e.set_chunk(4096)
        assert all(np.array_equal(p, q) for p, q in zip(a, c))
        # launches per pass: the fused path saves the ~30 launches of the tails
        names = [e.lib.pmp_ktime_name(k).decode() for k in range(e.lib.pmp_ktime_classes())]
        counts = {}
        for on in (True, False):
            e.set_fusion(on)
            e.ktime_enable(0xFFFF)
            e.inference_pre_QBD(comp, 22, y[:8], u[:8], v[:8])
            counts[on] = sum(int(ln) for ln, _, _ in e.ktime().values())
            e.ktime_enable(0)
        assert counts[False] - counts[True] >= 28 and counts[True] <= 42, counts      # 67 -> 37 launches per (QT + MTT) pass
        assert len(names) >= 6
        if comp == "Luma":          # range stress: the clamp fires inside the fused kernels too - same clamped bits, same raised flag
            e.load("Luma", 22)
            e.load_pretrain_model("Luma_MSBD", 22, Y.range_stress_weights())
            e.set_saturation_policy("ignore")
            e.set_activation_scales(False)                       # exponents of zero: the stress weights saturate
            got = {}
            for on in (True, False):
                e.set_fusion(on)
                e.clear_saturation()
                got[on] = e.inference_pre_QBD("Luma", 22, y[:6])
                assert e.saturated()
            assert all(np.array_equal(p, q) for p, q in zip(got[True], got[False]))
    finally:
        e.close()


def test_product_library_ships_no_winograd_form():
    """The Winograd-x form of the 3x3 64->64 convolutions (conv_f16x3_wx.hip) did not beat the direct kernels, so - like every other form
    that lost its A/B - it is built into the measurement library only: the product library accepts "off" and refuses "on".  Its parity
    checks (logits vs the oracle, flags bit-exact, range guard through it) run in tools/wx_probe.py against libpmp_hip_abl.so."""
    from pmp_vvc_tip2023_amd import _lib, engine
    e2 = engine.Engine(0, allow_synthetic_mtt=True)
    try:
        assert e2.lib.pmp_debug_set_winograd(e2.h, 0) == 0
        assert e2.lib.pmp_debug_set_winograd(e2.h, 1) == -1           # PMP_E_INVALID
        assert b"libpmp_hip_abl.so" in e2.lib.pmp_last_error(e2.h)
    finally:
        e2.close()


# ------------------------------------------------------------------------------------------------ post-processing
def test_map_to_partition_bit_exact_vs_reference_golden(eng, oracle_lib):
    """G3 through pmp_postprocess.  The ABI applies eli_structual_error first (as seq_post_process does), so golden
    outputs are compared where the fix is the identity on the fixture's QT map; the rest goes against the oracle."""
    n_gold = n_oracle = 0
    for tag, cf, qt, bt, dire, hor, ver, dout, leaves in g3_sets():
        comp = "Luma" if cf == 1 else "Chroma"
        h, v, q8, d8 = eng.post_process(qt, bt, dire, comp)
        fixed = oracle_lib.eli_structural_error(qt).reshape(-1, 8, 8)
        assert np.array_equal(q8, fixed.astype(np.uint8)), (tag, cf)
        same = np.all(fixed == qt, axis=(1, 2))
        assert np.array_equal(h[same], hor[same]) and np.array_equal(v[same], ver[same]) and np.array_equal(d8[same], dout[same]), (tag, cf)
        n_gold += int(same.sum())
        if (~same).any():
            oh, ov, od, _ = oracle_lib.map_to_partition(fixed[~same], bt[~same], dire[~same], cf)
            assert np.array_equal(h[~same], oh) and np.array_equal(v[~same], ov) and np.array_equal(d8[~same], od), (tag, cf)
            n_oracle += int((~same).sum())
    assert n_gold >= 1900 and n_oracle > 0        # 2204 reference triples; the few with a QT map the fix changes go against the oracle


def test_eli_structural_error_bit_exact(eng):
    g = golden("g4_eli.npz")
    n = g["qt"].shape[0]
    z = np.zeros((n, 3, 16, 16), np.float32)
    _, _, q8, _ = eng.post_process(g["qt"], z, z, "Luma")
    assert np.array_equal(q8.reshape(n, 1, 8, 8), g["out"].astype(np.uint8))


@pytest.mark.parametrize("comp", ["Luma", "Chroma"])
def test_seq_post_process_file_bytes(eng, comp, tmp_path):
    """G5: reference seq_post_process output file, byte for byte."""
    g = golden("g5_seq_%s.npz" % comp)
    p = str(tmp_path / "o.txt")
    eng.seq_post_process(g["qt"], g["bt"], g["dire"], comp, int(g["F"]), int(g["W"]), int(g["H"]), p)
    assert open(p, "rb").read() == open(golden_path("g5_partitionmat_%s.txt" % comp), "rb").read()


def test_postprocess_large_random_vs_oracle(eng, oracle_lib):
    """20k fresh triples (valid partitions + noise, both chroma factors) against the pinned oracle."""
    from pmp_vvc_tip2023_amd import synth
    for cf, comp in ((1, "Luma"), (2, "Chroma")):
        qt, bt, dire = synth.random_partition_batch(10000, 4242 + cf, cf, 0.2)
        rng = np.random.default_rng(cf)
        qt_logits = (qt + rng.normal(0, 0.3, qt.shape)).astype(np.float32)   # eli has real work to do
        h, v, q8, d8 = eng.post_process(qt_logits, bt, dire, comp)
        fixed = oracle_lib.eli_structural_error(qt_logits).reshape(-1, 8, 8)
        oh, ov, od, _ = oracle_lib.map_to_partition(fixed, bt, dire, cf)
        assert np.array_equal(q8, fixed.astype(np.uint8))
        assert np.array_equal(h, oh) and np.array_equal(v, ov) and np.array_equal(d8, od)
        assert h[:, 0, :].all() and v[:, :, 0].all()       # block top row / left column are always edges


def test_postprocess_value_range_bit_exact_vs_reference_golden(eng):
    """G3b: the REFERENCE's eli_structual_error + map_to_parititon on what a net with trained-scale activations can
    hand over - depth / direction logits of 50, 99.5, 100, 100.5, 300, 1e4, 3e38 and their negatives, QT logits of +-1e4 - and on +-inf
    and NaN in every input.  np.round has no clamp (Map2Partition.py:104); the kernel's integer copy of the rounded depth saturates at
    +-100 (postproc.hip: Search::mb) and must not differ anywhere.  Host-pointer, device-pointer and record entry points."""
    dev = torch.device("cuda:0")
    for cf, qt, bt, dire, tags, fixed, q8g, hor, ver, dout, leaves in g3b_sets():
        comp = "Luma" if cf == 1 else "Chroma"
        n = len(qt)
        h, v, q8, d8 = eng.post_process(qt, bt, dire, comp)
        for t in np.unique(tags):
            m = tags == t
            assert np.array_equal(q8[m], q8g[m]), (cf, t, "qt")
            assert np.array_equal(h[m], hor[m]) and np.array_equal(v[m], ver[m]), (cf, t, "edges")
            assert np.array_equal(d8[m], dout[m]), (cf, t, "dire")
        d_in = [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (qt, bt, dire)]
        d_h = torch.empty((n, 16, 16), dtype=torch.uint8, device=dev); d_v = torch.empty_like(d_h)
        d_q = torch.empty((n, 8, 8), dtype=torch.uint8, device=dev); d_d = torch.empty((n, 3, 16, 16), dtype=torch.int8, device=dev)
        eng.postprocess_device(comp, d_in[0].data_ptr(), d_in[1].data_ptr(), d_in[2].data_ptr(), n, d_h.data_ptr(), d_v.data_ptr(),
                               d_q.data_ptr(), d_d.data_ptr())
        rec = torch.empty((n, 1344), dtype=torch.uint8, device=dev)
        eng.postprocess_records_device(comp, d_in[0].data_ptr(), d_in[1].data_ptr(), d_in[2].data_ptr(), n, rec.data_ptr())
        eng.synchronize()
        assert np.array_equal(d_h.cpu().numpy(), hor) and np.array_equal(d_v.cpu().numpy(), ver)
        assert np.array_equal(d_q.cpu().numpy(), q8g) and np.array_equal(d_d.cpu().numpy(), dout)
        r = rec.cpu().numpy()
        assert np.array_equal(r[:, :256].reshape(n, 16, 16), hor) and np.array_equal(r[:, 256:512].reshape(n, 16, 16), ver)
        assert np.array_equal(r[:, 512:576].reshape(n, 8, 8), q8g) and np.array_equal(r[:, 576:].view(np.int8).reshape(n, 3, 16, 16), dout)


def test_postprocess_random_bit_patterns_vs_oracle(eng, oracle_lib):
    """"Every float32 bit pattern" taken literally: 3000 triples per chroma factor whose logits are raw random bits (NaNs with payloads,
    denormals, 1e38s, both zeros - a third of them pure noise, the rest valid partitions with 5..30 % of their cells replaced) against the
    oracle, which G3b's "bits" triples and tests/test_oracle_postproc.py pin on the reference for exactly this kind of input."""
    from pmp_vvc_tip2023_amd import synth
    for cf, comp in ((1, "Luma"), (2, "Chroma")):
        rng = np.random.default_rng(9000 + cf)
        n = 3000

        def bits(shape):
            return rng.integers(0, 2 ** 32, size=shape, dtype=np.uint64).astype(np.uint32).view(np.float32)
        qt, bt, dire = synth.random_partition_batch(n, 777 + cf, cf, 0.2)
        qt = (qt + rng.normal(0, 0.25, qt.shape)).astype(np.float32)
        frac = rng.choice([0.05, 0.1, 0.3, 1.0], size=n, p=[0.25, 0.25, 0.17, 0.33])
        for arr in (qt, bt, dire):
            m = rng.random(arr.shape) < frac.reshape((n,) + (1,) * (arr.ndim - 1))
            arr[m] = bits(int(m.sum()))
        h, v, q8, d8 = eng.post_process(qt, bt, dire, comp)
        with np.errstate(invalid="ignore"):
            fixed = oracle_lib.eli_structural_error(qt).reshape(-1, 8, 8)
            oh, ov, od, _ = oracle_lib.map_to_partition(fixed, bt, dire, cf)
            assert np.array_equal(q8, np.nan_to_num(fixed, nan=0.0).astype(np.uint8))
        assert np.array_equal(h, oh) and np.array_equal(v, ov) and np.array_equal(d8, od)
        assert np.isnan(fixed).any() and not np.isfinite(bt).all()


def test_fused_path_on_overflowing_nets_matches_the_oracle_on_its_own_logits(eng, g1, oracle_lib):
    """Logits that really come out of the nets beyond every sane range: MTT weights whose stem is scaled by 2^17 with the activation scales
    off (f16x3 under PMP_SAT_IGNORE: clamped activations, wrong but finite logits), and head biases of +inf / NaN / -inf (every datapath:
    the heads are fp32 kernels, so out0's depth plane is +inf, its direction plane NaN, out1 accumulates the +inf, out2's planes are
    -inf / +inf - and the attention inputs built from them carry the NaN into the trunks).  Whatever the logits are, the flags of the
    fused entry point must be the reference's post-processing OF THOSE LOGITS (oracle pinned on non-finite values by G3b).
    (Non-finite ACTIVATIONS are outside every datapath's domain: the kernels' ReLU is max(v, 0), which maps NaN to 0 where torch keeps it.)"""
    from pmp_vvc_tip2023_amd import engine
    y = np.ascontiguousarray(g1["block_y"][:8])
    e2 = engine.Engine(0, allow_synthetic_mtt=True)
    try:
        e2.set_precision(eng.get_precision())
        e2.load("Luma", 22)
        e2.set_activation_scales(False)
        e2.set_saturation_policy("ignore")
        for case in ("stem_x_2^17", "head_biases_nonfinite"):
            w = Y.range_stress_weights(2.0 ** 17 if case == "stem_x_2^17" else 1.0)
            if case == "head_biases_nonfinite":
                w["conv_B1.bias"] = np.array([np.inf, np.nan], np.float32)
                w["conv_B3.bias"] = np.array([-np.inf, np.inf], np.float32)
            e2.load_pretrain_model("Luma_MSBD", 22, w)
            hor, ver, q8, d8, qt, bt, dire = e2.infer_postprocess("Luma", 22, y, want_logits=True)
            if case == "head_biases_nonfinite":
                assert np.isposinf(bt[:, 0]).all() and np.isnan(dire[:, 0]).all() and np.isposinf(bt[:, 1]).all()
                assert not np.isfinite(bt[:, 2]).any() and not np.isfinite(dire[:, 2]).any()      # -inf / +inf, or NaN where the trunk fed NaN into the head
            assert Y.flags_equal((hor, ver, q8, d8), Y.oracle_flags("Luma", qt, bt, dire), nan_to_zero=True), case
    finally:
        e2.close()


# ------------------------------------------------------------------------------------------------ cutter
@pytest.mark.parametrize("bd", [8, 10])
def test_block_cutter_vs_reference_golden(eng, bd):
    g = golden("g6_cut.npz")
    by, bu, bv = eng.output_block_yuv(g["y%d" % bd], g["u%d" % bd], g["v%d" % bd], bd)
    assert np.array_equal(by, g["by%d" % bd]) and np.array_equal(bu, g["bu%d" % bd]) and np.array_equal(bv, g["bv%d" % bd])


def test_block_cutter_1080p_vs_oracle(eng, oracle_lib):
    from pmp_vvc_tip2023_amd import synth
    y, u, v = synth.recipe_r_frames(1, 1080, 1920, 3, bitdepth=10)
    by, bu, bv = eng.output_block_yuv(y, u, v, 10)
    oy, ou, ov = oracle_lib.cut_blocks(y, u, v, 10)
    assert by.shape == (480, 68, 68)                       # 30 x 16 blocks, bottom 56 rows dropped
    assert np.array_equal(by, oy) and np.array_equal(bu, ou) and np.array_equal(bv, ov)
    # tiny frame: fewer than 64 rows -> no blocks
    e = eng.output_block_yuv(np.zeros((1, 32, 128), np.uint8), np.zeros((1, 16, 64), np.uint8), np.zeros((1, 16, 64), np.uint8), 8)
    assert e[0].shape == (0, 68, 68)


def test_block_cutter_8k_frame_vs_oracle(eng, oracle_lib):
    """The largest picture a VVC level admits here: one 7680x4320 frame, 8040 blocks, 10-bit (the half-even reduction on 33 M samples) and
    8-bit, host-pointer seam - byte for byte the oracle's cutter (Inference_QBD.py:104-149)."""
    rng = np.random.default_rng(8)
    y = rng.integers(0, 1024, size=(1, 4320, 7680), dtype=np.uint16)
    u = rng.integers(0, 1024, size=(1, 2160, 3840), dtype=np.uint16)
    v = rng.integers(0, 1024, size=(1, 2160, 3840), dtype=np.uint16)
    for bd, (a, b, c) in ((10, (y, u, v)), (8, tuple((t & 255).astype(np.uint8) for t in (y, u, v)))):
        by, bu, bv = eng.output_block_yuv(a, b, c, bd)
        oy, ou, ov = oracle_lib.cut_blocks(a, b, c, bd)
        assert by.shape == (120 * 67, 68, 68) and np.array_equal(by, oy) and np.array_equal(bu, ou) and np.array_equal(bv, ov), bd


# ------------------------------------------------------------------------------------------------ full path, full size
def test_config2_full_batch_properties(eng, oracle_lib):
    """BASELINE.json configs[1] size (1024 luma CTUs = 4096 blocks, QP22: one bench.py step), device-resident fused path:
    * fused infer+postprocess == postprocess(infer) bit for bit, and is deterministic across runs
    * split flags are bit-exact against the oracle post-processing of the SAME device logits
    * logits of a 24-block sample within 1e-3 of the torch oracle
    * invariants of every valid partition (block borders are edges, QT map 2x2-constant, dire in {-1,0,1})."""
    from pmp_vvc_tip2023_amd import synth
    n = 4096
    y, u, v = synth.recipe_r_blocks(n, 1)
    eng.load("Luma", 22)
    dev = torch.device("cuda:0")
    d_y = torch.from_numpy(y).to(dev)
    outs = []
    for _ in range(2):
        hor = torch.empty((n, 16, 16), dtype=torch.uint8, device=dev); ver = torch.empty_like(hor)
        q8 = torch.empty((n, 8, 8), dtype=torch.uint8, device=dev); d8 = torch.empty((n, 3, 16, 16), dtype=torch.int8, device=dev)
        qt = torch.empty((n, 1, 8, 8), device=dev); bt = torch.empty((n, 3, 16, 16), device=dev); dire = torch.empty_like(bt)
        eng.infer_postprocess_device("Luma", 22, d_y.data_ptr(), None, None, n, hor.data_ptr(), ver.data_ptr(), q8.data_ptr(),
                                     d8.data_ptr(), qt.data_ptr(), bt.data_ptr(), dire.data_ptr())
        eng.synchronize()
        outs.append([t.cpu().numpy() for t in (hor, ver, q8, d8, qt, bt, dire)])
    for a, b in zip(outs[0], outs[1]):
        assert np.array_equal(a, b)
    assert not eng.saturated() and eng.saturation_reruns() == 0   # configs[1] stays far inside the f16x3 range: no re-run
    assert eng.workspace_bytes() <= {"f16x3": 2.75, "bf16x6": 4.1, "fp32": 2.75}[eng.get_precision()] * 2 ** 20 * n   # arena reuse
    hor, ver, q8, d8, qt, bt, dire = outs[0]
    h2, v2, q82, d82 = eng.post_process(qt, bt, dire, "Luma")
    assert np.array_equal(hor, h2) and np.array_equal(ver, v2) and np.array_equal(q8, q82) and np.array_equal(d8, d82)
    assert Y.flags_equal((hor, ver, q8, d8), Y.oracle_flags("Luma", qt, bt, dire))
    assert hor[:, 0, :].all() and ver[:, :, 0].all()
    assert np.array_equal(q8[:, ::2, ::2], q8[:, 1::2, 1::2]) and q8.max() <= 3 and set(np.unique(d8)) <= {-1, 0, 1}
    idx = np.arange(0, n, n // 24)[:24]
    o_q, o_bt, o_dire = Y.oracle_logits("Luma", 22, y[idx])
    assert np.abs(qt[idx] - o_q).max() < TOL and np.abs(bt[idx] - o_bt).max() < TOL and np.abs(dire[idx] - o_dire).max() < TOL


def test_config3_1080p_frame_all_qps(eng, oracle_lib, tmp_path):
    """BASELINE.json configs[2]: one synthetic 1920x1080 frame -> 480 blocks, luma+chroma x 4 QPs; emitted file equals
    the oracle's post-processing + writer on the same device logits, byte for byte."""
    from pmp_vvc_tip2023_amd import synth
    y, u, v = synth.recipe_r_frames(1, 1080, 1920, 3)
    by, bu, bv = eng.output_block_yuv(y, u, v, 8)
    for comp in ("Luma", "Chroma"):
        for qp in (22, 27, 32, 37):
            qt, bt, dire = eng.inference_pre_QBD(comp, qp, by, bu, bv)
            p = str(tmp_path / ("%s_%d.txt" % (comp, qp)))
            eng.seq_post_process(qt, bt, dire, comp, 1, 1920, 1080, p)
            po = str(tmp_path / ("o_%s_%d.txt" % (comp, qp)))
            oracle_lib.seq_post_process(qt, bt, dire, comp, 1, 1920, 1080, po)
            a, b = open(p, "rb").read(), open(po, "rb").read()
            assert a == b and a.count(b"\n") == 645120


# ------------------------------------------------------------------------------------------------ driver end to end
def test_driver_end_to_end_files(eng, oracle_lib, tmp_path):
    """The CLI driver on two tiny synthetic sequences (8-bit 192x128 and 10-bit 136x72, temporal sub-sampling 2):
    every emitted PartitionMat file equals oracle(cutter) -> HIP logits -> oracle(post-processing + writer), and
    the Time_Sta log has the reference's shape (Inference_QBD.py:243-253)."""
    import os
    from pmp_vvc_tip2023_amd import inference_qbd as D, synth
    inp = tmp_path / "in"; out = tmp_path / "out"; cfg = tmp_path / "cfg"
    inp.mkdir(); cfg.mkdir()
    seqs = [("SeqA", "SeqA_192x128_30.yuv", 192, 128, 3, 8), ("SeqB", "SeqB_136x72_30.yuv", 136, 72, 4, 10)]
    with open(inp / "table.txt", "w") as f:
        for name, fn, w, h, fr, bd in seqs:
            f.write("%s,%s,%d,%d,%d,30\n" % (name, fn, w, h, fr))
        f.write("#end!!!!\n")
    planes = {}
    for k, (name, fn, w, h, fr, bd) in enumerate(seqs):
        y, u, v = synth.recipe_r_frames(fr, h, w, 70 + k, bitdepth=bd)
        planes[name] = (y, u, v)
        with open(inp / fn, "wb") as f:
            for i in range(fr):
                f.write(y[i].tobytes()); f.write(u[i].tobytes()); f.write(v[i].tobytes())
        with open(cfg / (name + ".cfg"), "w") as f:
            f.write("InputFile                     : %s   # comment\nInputBitDepth                 : %d\n" % (fn, bd))
    D.main(["--jobID", "j1", "--inputDir", str(inp), "--outDir", str(out), "--seqTable", "table.txt", "--cfgDir", str(cfg),
            "--ssRatio", "2", "--startSeqID", "0", "--seqNum", "2", "--batchSize", "5", "--strictBatch", "--qps", "22,37", "--binary",
            "--allowSyntheticMTT"])
    for name, fn, w, h, fr, bd in seqs:
        y, u, v = planes[name]
        by, bu, bv = oracle_lib.cut_blocks(y[::2], u[::2], v[::2], bd)
        nf = (fr + 1) // 2
        for comp in ("Luma", "Chroma"):
            for qp in (22, 37):
                qt, bt, dire = eng.inference_pre_QBD(comp, qp, by, bu, bv)
                po = str(tmp_path / "o.txt")
                oracle_lib.seq_post_process(qt, bt, dire, comp, nf, w, h, po)
                got = out / "j1" / "PartitionMat" / ("%s_%s_QP%d_PartitionMat.txt" % (fn[:-4], comp, qp))
                assert open(got, "rb").read() == open(po, "rb").read(), (name, comp, qp)
                # --binary: the side-channel file next to it holds the same numbers
                from pmp_vvc_tip2023_amd import engine as E
                f_, h_, w_, bh_, bv_, bq_, bd_ = E.read_partition_binary(str(got)[:-4] + ".pmpb")
                th_, tv_, tq_, td_ = E.read_partition_file(str(got), nf, h, w)
                assert (f_, h_, w_) == (nf, h, w) and np.array_equal(bh_, th_) and np.array_equal(bv_, tv_)
                assert np.array_equal(bq_, tq_) and np.array_equal(bd_, td_)
    rows = open(out / "j1" / "Time_Sta_0_2.txt").read().strip().split("\n")
    assert len(rows) == 2 * 4 and all(r.count(",") == 5 for r in rows)
    # the default run kept the blocks device-resident; the reference-style host block arrays give the same bytes
    out2 = tmp_path / "out_host"
    D.main(["--jobID", "j1", "--inputDir", str(inp), "--outDir", str(out2), "--seqTable", "table.txt", "--cfgDir", str(cfg),
            "--ssRatio", "2", "--startSeqID", "0", "--seqNum", "2", "--batchSize", "5", "--qps", "22,37", "--hostBlocks", "--allowSyntheticMTT"])
    names = sorted(n for n in os.listdir(out / "j1" / "PartitionMat") if n.endswith(".txt"))
    assert names == sorted(os.listdir(out2 / "j1" / "PartitionMat")) and len(names) == 8
    for nm in names:
        assert open(out / "j1" / "PartitionMat" / nm, "rb").read() == open(out2 / "j1" / "PartitionMat" / nm, "rb").read(), nm


def test_driver_overlap_mode_is_byte_identical(tmp_path):
    """The CLI driver's --overlap turns the library's overlap mode on (opt-in since round 6): passes of >= 1024 blocks run as two chunks
    on two streams.  A sequence large enough to be cut (2 frames of 2048x1088 = 1088 blocks per pass) gives the same files either way."""
    import os
    from pmp_vvc_tip2023_amd import inference_qbd as D, synth
    inp = tmp_path / "in"; cfg = tmp_path / "cfg"
    inp.mkdir(); cfg.mkdir()
    w, h, fr = 2048, 1088, 2
    with open(inp / "table.txt", "w") as f:
        f.write("SeqO,SeqO_2048x1088_30.yuv,%d,%d,%d,30\n#end!!!!\n" % (w, h, fr))
    y, u, v = synth.recipe_r_frames(fr, h, w, 91)
    with open(inp / "SeqO_2048x1088_30.yuv", "wb") as f:
        for i in range(fr):
            f.write(y[i].tobytes()); f.write(u[i].tobytes()); f.write(v[i].tobytes())
    with open(cfg / "SeqO.cfg", "w") as f:
        f.write("InputFile                     : SeqO_2048x1088_30.yuv\nInputBitDepth                 : 8\n")
    outs = {}
    for tag, extra in (("on", ["--overlap"]), ("off", [])):
        out = tmp_path / ("out_" + tag)
        D.main(["--jobID", "j", "--inputDir", str(inp), "--outDir", str(out), "--seqTable", "table.txt", "--cfgDir", str(cfg), "--ssRatio", "1",
                "--startSeqID", "0", "--seqNum", "1", "--qps", "22,32", "--allowSyntheticMTT"] + extra)
        d = out / "j" / "PartitionMat"
        outs[tag] = {n: open(d / n, "rb").read() for n in sorted(os.listdir(d))}
    assert len(outs["on"]) == 4 and list(outs["on"]) == list(outs["off"])
    for n in outs["on"]:
        assert outs["on"][n] == outs["off"][n], n
        assert outs["on"][n].count(b"\n") == fr * (5 * (16 * 17) * (16 * 32) + (8 * 17) * (8 * 32))


def test_config4_4k_frame_sharded_equals_unsharded(eng, oracle_lib):
    """BASELINE.json configs[3] on one GPU: a synthetic 3840x2160 frame (1980 blocks).  Processing the block stream in the
    contiguous shards 8 ranks would take (parallel.shard_bounds) and concatenating the records gives the same bytes as
    one pass - the multi-GPU path has no cross-block dependency - and the emitted file passes the format invariants."""
    from pmp_vvc_tip2023_amd import engine as E, parallel, synth
    y, u, v = synth.recipe_r_frames(1, 2160, 3840, 4)
    by, bu, bv = eng.output_block_yuv(y, u, v, 8)
    n = by.shape[0]
    assert n == 60 * 33
    for comp, qp in (("Luma", 32), ("Chroma", 27)):
        whole = parallel.pack_records(*eng.infer_postprocess(comp, qp, by, bu, bv))
        parts = []
        for r in range(8):
            lo, hi = parallel.shard_bounds(n, r, 8)
            parts.append(parallel.pack_records(*eng.infer_postprocess(comp, qp, by[lo:hi], bu[lo:hi], bv[lo:hi])))
        assert np.array_equal(np.concatenate(parts), whole)
        h, vv, q8, d8 = parallel.unpack_records(whole)
        text = E.format_partition_text(1, 2160, 3840, h, vv, q8, d8)
        assert text.count(b"\n") == 5 * (33 * 16) * (60 * 16) + (33 * 8) * (60 * 8)
        assert h.reshape(33, 60, 16, 16)[:, :, 0, :].all() and vv.reshape(33, 60, 16, 16)[:, :, :, 0].all()


def test_driver_sequence_without_a_full_block(tmp_path):
    """A sequence smaller than one 64x64 block (the reference's (H // 64) * (W // 64) = 0, Inference_QBD.py:125-129 cuts nothing):
    the driver writes EMPTY PartitionMat files - what get_sequence_partition_for_VTM's loops produce for zero rows - and does not fail."""
    import os
    from pmp_vvc_tip2023_amd import inference_qbd as D
    inp = tmp_path / "in"; cfg = tmp_path / "cfg"
    inp.mkdir(); cfg.mkdir()
    w, h, fr = 96, 48, 2
    with open(inp / "Small_96x48_30.yuv", "wb") as f:
        f.write(bytes(fr * w * h * 3 // 2))
    (inp / "table.txt").write_text("Small,Small_96x48_30.yuv,%d,%d,%d,30\n#end!!!!\n" % (w, h, fr))
    (cfg / "Small.cfg").write_text("InputFile : Small_96x48_30.yuv\nInputBitDepth : 8\n")
    D.main(["--jobID", "s", "--inputDir", str(inp), "--outDir", str(tmp_path / "o"), "--seqTable", "table.txt", "--cfgDir", str(cfg),
            "--ssRatio", "1", "--seqNum", "1", "--qps", "22", "--allowSyntheticMTT", "--binary"])
    pm = tmp_path / "o" / "s" / "PartitionMat"
    for comp in ("Luma", "Chroma"):
        assert os.path.getsize(pm / ("Small_96x48_30_%s_QP22_PartitionMat.txt" % comp)) == 0
        assert os.path.getsize(pm / ("Small_96x48_30_%s_QP22_PartitionMat.pmpb" % comp)) == 40      # header only


def test_config4_eight_4k_frames_all_qps_through_the_driver(tmp_path):
    """BASELINE.json configs[3]'s input on the one GPU of the test box: 8 synthetic 3840x2160 frames, Luma + Chroma x 4 QPs through the
    CLI driver (device-resident blocks, packed records, writer threads).  Every file has the geometry the VTM parser expects
    (EncAppCfg.cpp:4243-4250: 528 x 960 cells, 8 frames) and the partition invariants; and because frames are independent, frame 5
    of the 8-frame files equals the file a one-frame sequence made of that frame gives - the property the frame-sharded
    multi-GPU run rests on (tests/test_parallel_cpu.py covers the gather itself)."""
    import os
    from pmp_vvc_tip2023_amd import inference_qbd as D, synth
    W_, H_, F_ = 3840, 2160, 8
    y, u, v = synth.recipe_r_frames(F_, H_, W_, 4)
    inp = tmp_path / "in"; cfg = tmp_path / "cfg"
    inp.mkdir(); cfg.mkdir()
    for name, frames in (("All", range(F_)), ("One", [5])):
        fn = "%s_3840x2160_30.yuv" % name
        with open(inp / fn, "wb") as f:
            for i in frames:
                f.write(y[i].tobytes()); f.write(u[i].tobytes()); f.write(v[i].tobytes())
        (cfg / (name + ".cfg")).write_text("InputFile : %s\nInputBitDepth : 8\n" % fn)
    (inp / "table.txt").write_text("All,All_3840x2160_30.yuv,3840,2160,8,30\nOne,One_3840x2160_30.yuv,3840,2160,1,30\n#end!!!!\n")
    D.main(["--jobID", "c4", "--inputDir", str(inp), "--outDir", str(tmp_path / "out"), "--seqTable", "table.txt", "--cfgDir", str(cfg),
            "--ssRatio", "1", "--seqNum", "2", "--allowSyntheticMTT"])
    pm = tmp_path / "out" / "c4" / "PartitionMat"
    per_frame = 5 * 528 * 960 + 264 * 480                   # lines per frame
    for comp in ("Luma", "Chroma"):
        for qp in (22, 27, 32, 37):
            allf = open(pm / ("All_3840x2160_30_%s_QP%d_PartitionMat.txt" % (comp, qp)), "rb").read()
            one = open(pm / ("One_3840x2160_30_%s_QP%d_PartitionMat.txt" % (comp, qp)), "rb").read()
            assert allf.count(b"\n") == F_ * per_frame and one.count(b"\n") == per_frame
            # frame 5 of the long file: skip five frames' worth of lines
            pos = 0
            for _ in range(5 * per_frame):
                pos = allf.index(b"\n", pos) + 1
            assert allf[pos:pos + len(one)] == one, (comp, qp)
    hor, ver, qt, dire = E_read(pm / "All_3840x2160_30_Luma_QP32_PartitionMat.txt", F_, H_, W_)
    assert hor[:, ::16, :].all() and ver[:, :, ::16].all()  # block borders are edges in every frame
    assert qt.max() <= 3 and set(np.unique(dire)) <= {-1, 0, 1}


def E_read(path, frames, height, width):
    from pmp_vvc_tip2023_amd import engine as E
    return E.read_partition_file(str(path), frames, height, width)


def test_end_to_end_flags_vs_reference_logits(eng, g1, oracle_lib):
    """End-to-end audit ('bit-exact flags is only well-defined for identical logits'): split flags
    from the HIP path (own logits) against flags the oracle derives from the REFERENCE's logits (G1/G2, torch CPU).
    |logit difference| is ~1e-5, so a pooled cell would have to sit that close to a .5 rounding boundary to flip;
    on the golden set none does, in either datapath."""
    g2 = golden("g2_msbd.npz")
    mism = total = 0
    for comp in ("Luma", "Chroma"):
        for qp in (22, 27, 32, 37):
            hor, ver, q8, d8 = eng.infer_postprocess(comp, qp, g1["block_y"][:8], g1["block_u"][:8], g1["block_v"][:8])
            qt_ref = g1["qt_%s_%d" % (comp, qp)][:8]
            bt_ref = np.stack([g2["out%d_%s_%d" % (k, comp, qp)][:, 0] for k in range(3)], 1)
            dr_ref = np.stack([g2["out%d_%s_%d" % (k, comp, qp)][:, 1] for k in range(3)], 1)
            oh, ov, oq, od = oracle_lib.seq_post_process(qt_ref, bt_ref, dr_ref, comp, 1, 64 * 8, 64, None)
            mism += int((hor != oh).sum() + (ver != ov).sum() + (q8 != oq.astype(np.uint8)).sum() + (d8 != od).sum())
            total += hor.size + ver.size + q8.size + d8.size
    assert total == 8 * 8 * 1344
    assert mism == 0, "%d of %d emitted values differ from the reference-logit path" % (mism, total)


def test_driver_two_ranks_equal_one_rank(tmp_path):
    """The sharded driver (2 processes: block rows split between them, each rank formats and pwrites its own rows, the ranks
    exchange only byte counts) writes the same files as a single process.  Both ranks share the one GPU of the test box, so the collective runs over gloo here; on a multi-GPU node the
    same code path uses RCCL."""
    import os, socket, subprocess, sys
    from pmp_vvc_tip2023_amd import inference_qbd as D, synth
    inp = tmp_path / "in"; cfg = tmp_path / "cfg"
    inp.mkdir(); cfg.mkdir()
    w, h, fr = 320, 192, 3                                   # 5 x 3 blocks per frame, 3 frames -> 45 blocks, odd split
    with open(inp / "table.txt", "w") as f:
        f.write("SeqC,SeqC_320x192_30.yuv,%d,%d,%d,30\n#end!!!!\n" % (w, h, fr))
    y, u, v = synth.recipe_r_frames(fr, h, w, 91)
    with open(inp / "SeqC_320x192_30.yuv", "wb") as f:
        for i in range(fr):
            f.write(y[i].tobytes()); f.write(u[i].tobytes()); f.write(v[i].tobytes())
    with open(cfg / "SeqC.cfg", "w") as f:
        f.write("InputFile : SeqC_320x192_30.yuv\nInputBitDepth : 8\n")
    common = ["--inputDir", str(inp), "--seqTable", "table.txt", "--cfgDir", str(cfg), "--ssRatio", "1", "--seqNum", "1", "--qps", "22,32", "--allowSyntheticMTT"]
    D.main(["--jobID", "one", "--outDir", str(tmp_path / "o1")] + common)
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), WORLD_SIZE="2", PMP_DIST_BACKEND="gloo", PYTHONPATH=root)
    procs = [subprocess.Popen([sys.executable, "-m", "pmp_vvc_tip2023_amd.inference_qbd", "--jobID", "two", "--outDir", str(tmp_path / "o2")] + common,
                              env=dict(env, RANK=str(r), LOCAL_RANK=str(r)), cwd=root, stdout=subprocess.PIPE, stderr=subprocess.STDOUT) for r in range(2)]
    logs = [p.communicate(timeout=600)[0].decode() for p in procs]
    assert all(p.returncode == 0 for p in procs), "\n".join(logs)
    d1 = tmp_path / "o1" / "one" / "PartitionMat"; d2 = tmp_path / "o2" / "two" / "PartitionMat"
    names = sorted(os.listdir(d1))
    assert len(names) == 4 and names == sorted(os.listdir(d2))
    for nme in names:
        assert open(d1 / nme, "rb").read() == open(d2 / nme, "rb").read(), nme
    # --emit gather: the older path (records gathered to rank 0, which writes alone) gives the same bytes
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    env = dict(env, MASTER_PORT=str(port))
    procs = [subprocess.Popen([sys.executable, "-m", "pmp_vvc_tip2023_amd.inference_qbd", "--jobID", "g", "--outDir", str(tmp_path / "og"), "--emit", "gather"] + common,
                              env=dict(env, RANK=str(r), LOCAL_RANK=str(r)), cwd=root, stdout=subprocess.PIPE, stderr=subprocess.STDOUT) for r in range(2)]
    logs = [p.communicate(timeout=600)[0].decode() for p in procs]
    assert all(p.returncode == 0 for p in procs), "\n".join(logs)
    for nme in names:
        assert open(d1 / nme, "rb").read() == open(tmp_path / "og" / "g" / "PartitionMat" / nme, "rb").read(), nme
    # the driver as its own launcher: --gpus 2 with no WORLD_SIZE in the environment spawns the two ranks itself
    env3 = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT", "MASTER_ADDR")}
    env3.update(PMP_DIST_BACKEND="gloo", PYTHONPATH=root)
    r = subprocess.run([sys.executable, "-m", "pmp_vvc_tip2023_amd.inference_qbd", "--jobID", "three", "--outDir", str(tmp_path / "o3"), "--gpus", "2"] + common,
                       env=env3, cwd=root, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    d3 = tmp_path / "o3" / "three" / "PartitionMat"
    assert names == sorted(os.listdir(d3))
    for nme in names:
        assert open(d1 / nme, "rb").read() == open(d3 / nme, "rb").read(), nme


# ------------------------------------------------------------------------------------------------ bench.py contract
def test_bench_json_contract(tmp_path):
    """bench.py --full prints ONE JSON line with the driver's fields, the roofline of the dominant kernel class measured with HIP
    events on the launch stream, the CPU baseline of a bounded sample and the parity of that sample."""
    import json, os, subprocess, sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--steps", "2", "--warmup", "1", "--batch", "64",
                        "--cpu-sample", "8", "--full"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.strip()]
    assert len(lines) == 1
    d = json.loads(lines[0])
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
              "dtype", "data", "config", "roofline", "cpu_baseline"):
        assert k in d, k
    assert d["n_gpus"] == 1 and d["steps"] == 2 and d["warmup"] == 1 and d["unit"] == "CTU/s" and d["vs_baseline"] is None
    assert d["higher_is_better"] is True and d["scaling"] == "weak" and d["data"] == "synthetic" and "workload" in d["config"]
    rf = d["roofline"]
    assert rf["bound"] == "mfma" and rf["unit"] == "TFLOP/s" and 0 < rf["frac"] < 1 and abs(rf["frac"] - rf["achieved"] / rf["peak"]) < 1e-3
    cb = d["cpu_baseline"]
    assert cb["kind"] == "port" and cb["cores"] >= 1 and cb["value"] > 0 and "sample" in cb
    assert d["parity"]["logit_max_abs_err"] < 1e-3 and d["parity"]["flag_mismatch_vs_oracle_postproc_of_device_logits"] == 0
    assert d["value"] > 50 * cb["value"]   # sanity: the GPU path is not the CPU path
    # round 6: `traffic` is printed only when the committed PMC record was taken on THIS build of the kernel file (sha256 stamp), else null + why
    assert rf["traffic_source"] and (("THIS kernel build" in rf["traffic_source"]) == (rf["traffic"] is not None))
    fx = d["extra"]["fp32_exact"]               # round 6: the exact-arithmetic datapath (and the cost of a range-guard re-run), witnessed every run
    assert fx["dtype"] == "f32" and 0 < fx["ctu_per_s"] < d["value"] and fx["roofline"]["peak"] == 157.3
    assert 0 < fx["roofline"]["frac"] < 1 and abs(fx["roofline"]["frac"] - fx["roofline"]["achieved"] / 157.3) < 1e-3
    hv = rf["hbm_view"]                         # the same launches against the HBM roof: algorithmic bytes / measured launch time
    assert hv["unit"] == "GB/s" and hv["peak"] == 8000 and 0 < hv["frac"] < 1 and abs(hv["frac"] - hv["achieved"] / hv["peak"]) < 1e-3
    assert abs(hv["algorithmic_bytes_per_launch"] - rf["flop_per_launch"] / 73728.0 * 640) < 2
    e2e = d["e2e_host_buffers"]                 # the H2D/D2H-inclusive figure beside the device-resident one
    assert e2e["unit"] == "CTU/s" and 0 < e2e["value"] <= d["value"] * 1.5 and e2e["h2d_bytes_per_step"] == 64 * 68 * 68
    assert set(d["extra"]["luma_ctu_per_s_by_qp"]) == {"22", "27", "32", "37"} and d["extra"]["chroma_qp22_ctu_per_s"] > 0
    # round 5: the step on trained-like MTT weights (no fp32 re-run, with and without the stress gains), this GPU's clock / power during the
    # timed region, and what the whole host - not one calibrated process - does on the CPU path
    tl = d["extra"]["trained_like"]
    assert tl["saturation_reruns"] == 0 and tl["saturation_reruns_stress_k64_g16"] == 0 and tl["ms_per_step"] > 0
    assert len(tl["activation_exps"]) == 5 and tl["activation_exps_stress_k64_g16"][0] >= tl["activation_exps"][0] + 5
    assert "samples" in d["sensors"] and "sclk_mhz" in d["sensors"] and "power_w" in d["sensors"]
    ac = cb["all_cores"]
    assert "error" in ac or (ac["processes"] >= 1 and ac["blocks_per_s"] > 0 and "cpu_limits" in ac and cb["host_cores"] >= cb["cores"])


def test_bench_plain_run_times_the_steps_only(tmp_path):
    """A plain `bench.py` run (no --full) prints the same headline fields and the roofline of its timed steps, and takes none of the
    side measurements: no CPU baseline or parity sample, no host-buffer, chroma, per-QP, other-datapath or per-class runs."""
    import json, os, subprocess, sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--steps", "2", "--warmup", "1", "--batch", "64"],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.strip()]
    assert len(lines) == 1
    d = json.loads(lines[0])
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "roofline"):
        assert k in d, k
    assert d["steps"] == 2 and d["warmup"] == 1 and d["unit"] == "CTU/s" and d["dtype"] == "f16x3" and d["value"] > 0
    assert abs(d["value"] - 64 / 4.0 / (d["ms_per_step"] * 1e-3)) < 1e-3 * d["value"] + 0.1
    assert d["roofline"]["kernel"] == "conv_mfma_3x3_c64" and 0 < d["roofline"]["frac"] < 1
    assert d["cpu_baseline"] is None
    for k in ("parity", "extra", "e2e_host_buffers", "breakdown", "chroma_roofline"):
        assert k not in d, k
    assert "cpu_baseline:" not in r.stderr


def test_bench_launches_its_own_ranks(tmp_path):
    """`python bench.py --gpus 2` with no launcher starts two rank processes itself (fresh children, before the parent makes
    a GPU call) and prints ONE line with n_gpus = 2 and twice the blocks.  Both ranks share the test box's single GPU, so the
    collective runs over gloo here (PMP_DIST_BACKEND); on a multi-GPU node the same path gathers device tensors over RCCL."""
    import json, os, subprocess, sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, PMP_DIST_BACKEND="gloo")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "1", "--batch", "32",
                        "--cpu-sample", "0", "--no-extras"], capture_output=True, text=True, timeout=900, env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, r.stdout
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["config"]["blocks_per_gpu"] == 32 and d["config"]["global_blocks"] == 64 and d["scaling"] == "weak"
    assert d["value"] > 0 and d["cpu_baseline"] is None
    # the multi-GPU line says what the collective saw and cost ("if the N = 8 number disappoints there is nothing to say why")
    m = d["multi_gpu"]
    assert d["rccl_ranks"] == 2 and m["rccl_ranks"] == 2 and m["backend"] == "gloo" and m["gather_bytes_per_step"] == 2 * 32 * 1344
    assert m["gather_ms"] >= 0 and len(m["ms_per_step_by_rank"]) == 2 and all(t > 0 for t in m["ms_per_step_by_rank"])
    assert max(m["ms_per_step_by_rank"]) <= d["ms_per_step"] * 1.05 and m["preflight_ms"] > 0
    assert "preflight ok: 2 ranks" in r.stderr
    # the N = 1 line carries none of it
    r1 = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--steps", "1", "--warmup", "1", "--batch", "32", "--cpu-sample", "0",
                         "--no-extras"], capture_output=True, text=True, timeout=900, env=env)
    assert r1.returncode == 0, r1.stderr[-3000:]
    d1 = json.loads(r1.stdout.strip())
    assert "multi_gpu" not in d1 and "rccl_ranks" not in d1 and d1["n_gpus"] == 1


def test_bench_dump_outputs_are_the_timed_steps_flags(tmp_path):
    """`bench.py --dump-outputs DIR` writes the split flags of its last timed step: the arrays pmp_infer_postprocess returns for the
    same seeded blocks (recipe R seed 1, Luma QP22, default datapath), as float32, with the block index beside them."""
    import os, subprocess, sys
    from pmp_vvc_tip2023_amd import engine, synth
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    n = 48
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--steps", "2", "--warmup", "0", "--batch", str(n), "--cpu-sample", "0",
                        "--no-extras", "--dump-outputs", str(tmp_path / "out")], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    got = {k: np.load(tmp_path / "out" / (k + ".npy")) for k in ("hor", "ver", "qt", "dire", "block_index")}
    assert all(a.dtype == np.float32 for k, a in got.items() if k != "block_index") and got["block_index"].dtype == np.float64
    assert np.array_equal(got["block_index"], np.arange(n))
    y, u, v = synth.recipe_r_blocks(n, 1)
    e = engine.Engine(0, allow_synthetic_mtt=True)
    try:
        hor, ver, q8, d8 = e.infer_postprocess("Luma", 22, y)
    finally:
        e.close()
    for k, want, shape in (("hor", hor, (n, 16, 16)), ("ver", ver, (n, 16, 16)), ("qt", q8, (n, 8, 8)), ("dire", d8, (n, 3, 16, 16))):
        assert got[k].shape == shape and np.array_equal(got[k], want.reshape(shape).astype(np.float32)), k

def test_records_entry_point_equals_the_four_arrays(eng):
    """pmp_infer_postprocess_records_device writes hor | ver | qt | dire of every block as one 1344-byte record: the same bytes
    as the four dense arrays of pmp_infer_postprocess_device, packed (what the multi-GPU gather moves)."""
    from pmp_vvc_tip2023_amd import parallel, synth
    n = 37
    y, u, v = synth.recipe_r_blocks(n, 5)
    dev = torch.device("cuda:0")
    d_y, d_u, d_v = (torch.from_numpy(a).to(dev) for a in (y, u, v))
    for comp in ("Luma", "Chroma"):
        eng.load(comp, 32)
        rec = torch.zeros((n, 1344), dtype=torch.uint8, device=dev)
        pu, pv = (d_u.data_ptr(), d_v.data_ptr()) if comp == "Chroma" else (None, None)
        eng.infer_postprocess_records_device(comp, 32, d_y.data_ptr(), pu, pv, n, rec.data_ptr())
        eng.synchronize()
        hor, ver, q8, d8 = eng.infer_postprocess(comp, 32, y, u, v)
        assert np.array_equal(rec.cpu().numpy(), parallel.pack_records(hor, ver, q8, d8))
