"""Layer-local GPU checks: every launch of the four nets against a float64 recomputation from the GPU's own inputs, the fused kernels
tensor by tensor, poisoned workspaces, and block-order independence of the persistent kernels.

Taps (pmp_debug_get_tap, include/pmp.h) give each intermediate tensor exactly as its consumer read it; oracle/layers64.py recomputes
each launch in float64 with the bound its datapath's arithmetic allows (tests/test_layer_bound_cpu.py shows the bound is sharp)."""
import numpy as np
import pytest
import torch

import gpu_rig
import trained_like  # tools/trained_like.py: test-weight data
from oracle import layers64 as L, range_cases as RC, taps as T
from oracle.parity import range_stress_weights

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------------------------------------ helpers
_edge_blocks = RC.edge_blocks       # 13 edge-case blocks (oracle/range_cases.py; also the site-by-site range tests' source)
_taps_on, _tap = T.taps_on, T.tap   # oracle/taps.py, shared with tests/test_gpu_range_sites.py


def _poison(e, pattern):
    e._ck(e.lib.pmp_debug_poison_workspace(e.h, int(pattern)))


def _weights(comp, qp, mtt):
    from pmp_vvc_tip2023_amd import weights as W
    wq, _ = W.load_net_weights(comp + "_Q", qp)
    if mtt == "trained_like":
        wb = trained_like.msbd_weights(comp, qp)
    else:
        wb, _ = W.load_net_weights(comp + "_MSBD", qp, allow_synthetic=True)
    return wq, wb


def _all_names():
    """Every tap name the graph can record, from the float64 walk (layer outputs; heads are logits, not taps)."""
    from pmp_vvc_tip2023_amd import synth, weights as W
    names = []
    for comp in ("Luma",):
        y, u, v = synth.recipe_r_blocks(1, 1)
        wq, wb = _weights(comp, 22, "synthetic")
        taps = {}
        x = L.blocks64(True, y, u, v)
        for gen in (L.q_layers(taps.__getitem__, wq, True, x, "fp32"), L.msbd_layers(taps.__getitem__, wb, True, x, "fp32")):
            for lay in gen:
                taps[lay.name] = lay.ref
                names.append(lay.name)
    return [n for n in names if "head" not in n]


_MAXR = {}    # (datapath, layer class) -> largest ratio seen in this session


def _per_layer(e):
    e.set_fusion(False)                  # every tensor of the graph exists (the fused kernels keep some in LDS); fused: test below
    e.set_saturation_policy("ignore")    # taps skip a range-guard re-run: nothing may saturate, checked below


@pytest.fixture(scope="module", params=gpu_rig.DATAPATHS)
def eng(request):
    # poison 2: finite garbage (0x3C bytes) in every workspace before each pass: an unwritten pad channel shows
    with gpu_rig.engine(request.param, synthetic_mtt=True, threads=16, setup=_per_layer, poison=2) as e:
        yield e
    print("\nlayer-local max |gpu - ref64| / bound on %s (c_dp %g):" % (request.param, L.C_DP[request.param]))
    for (dp, cls), r in sorted(_MAXR.items()):
        if dp == request.param:
            print("  %-14s %.3f" % (cls, r))


# ------------------------------------------------------------------------------------------------ 1. layer-local parity
# Padded channels (C rounded up to 16) that a kernel may leave unwritten: none - every producer stores whole 16-channel groups with
# zeros beyond the real channels, so a stale or poisoned byte there is a finding.  The workspaces are poisoned (fixture above), so a pad
# channel that no kernel writes holds 0x3C bytes, not whatever zeros an earlier pass left behind.
@pytest.mark.parametrize("mtt", ["synthetic", "trained_like"])
@pytest.mark.parametrize("qp", [22, 37])
@pytest.mark.parametrize("comp", ["Luma", "Chroma"])
def test_every_launch_within_its_float64_bound(eng, comp, qp, mtt):
    dp = eng.get_precision()
    luma = comp == "Luma"
    y, u, v = _edge_blocks()
    wq, wb = _weights(comp, qp, mtt)
    eng.load(comp, qp, q_weights=wq, msbd_weights=wb)
    exps = eng.activation_report(comp, qp)["exps"] if dp == "f16x3" else [0] * 5
    _taps_on(eng, True)
    try:
        eng.clear_saturation()
        qt, bt, dire = eng.inference_pre_QBD(comp, qp, y, u, v)
        assert not eng.saturated()
        logits = {"q/head": qt.astype(np.float64)}
        for k in range(3):
            logits["bd/head%d" % k] = np.stack([bt[:, k], dire[:, k]], 1).astype(np.float64)
        cache = {}

        def get(name):
            if name in logits:
                return torch.from_numpy(logits[name])
            if name not in cache:
                got = _tap(eng, name)
                assert got is not None, "no tap " + name
                t, cr = got
                assert np.isfinite(t).all(), name
                assert not t[:, cr:].any(), "%s: padded channels hold %s" % (name, np.unique(t[:, cr:])[:4])
                cache[name] = torch.from_numpy(np.ascontiguousarray(t[:, :cr]))
            return cache[name]
        x = L.blocks64(luma, y, u, v)
        worst = []
        for gen in (L.q_layers(get, wq, luma, x, dp), L.msbd_layers(get, wb, luma, x, dp, exps)):
            for lay in gen:
                gpu = get(lay.name)
                assert gpu.shape == lay.ref.shape, (lay.name, gpu.shape, lay.ref.shape)
                r = L.ratio(gpu, lay)
                key = (dp, lay.cls)
                _MAXR[key] = max(_MAXR.get(key, 0.0), r)
                worst.append((r, lay.name))
        worst.sort(reverse=True)
        print("%s %s QP%d %s: worst layers %s" % (dp, comp, qp, mtt, ", ".join("%s %.3f" % (n, r) for r, n in worst[:3])))
        assert worst[0][0] <= 1.0, "%s %s QP%d %s: %s" % (dp, comp, qp, mtt, worst[:5])
    finally:
        _taps_on(eng, False)


# ------------------------------------------------------------------------------------------------ 2. fused kernels, tensor by tensor
@pytest.mark.parametrize("comp", ["Luma", "Chroma"])
def test_fusion_modes_agree_tensor_by_tensor(comp):
    """f16x3: every tensor that exists in fusion modes 0..3 is bit-identical across the modes (chain16.hip and rbfuse32.hip hand on
    q/resblock_q3, bd/trunk_Att1.1, trunk_B3.1, trunk_Att2.0 exactly as the launch-per-layer path writes them)."""
    from pmp_vvc_tip2023_amd import engine
    y, u, v = _edge_blocks()
    names = _all_names()
    e = engine.Engine(0, allow_synthetic_mtt=True)
    try:
        e.set_precision("f16x3")
        e.set_saturation_policy("ignore")
        for mtt in ("synthetic", "trained_like"):
            wq, wb = _weights(comp, 22, mtt)
            e.load(comp, 22, q_weights=wq, msbd_weights=wb)
            got = {}
            for mode in (0, 1, 2, 3):
                e.set_fusion(mode)
                _taps_on(e, True)
                e.clear_saturation()
                e.inference_pre_QBD(comp, 22, y, u, v)
                assert not e.saturated()
                got[mode] = {n: t for n, t in ((n, _tap(e, n)) for n in names) if t is not None}
                _taps_on(e, False)
            assert len(got[0]) == len(names)
            for must in ("q/resblock_q3", "bd/trunk_Att1.1", "bd/trunk_B3.1", "bd/trunk_Att2.0"):
                assert all(must in got[m] for m in (0, 1, 2, 3)), must
            for mode in (1, 2, 3):
                for n, (t, _) in got[mode].items():
                    assert np.array_equal(t, got[0][n][0]), "%s %s fusion %d: %s differs by %g" % (comp, mtt, mode, n, np.abs(t - got[0][n][0]).max())
    finally:
        e.close()


# ------------------------------------------------------------------------------------------------ 3. poisoned workspaces
@pytest.mark.parametrize("dp,fusion", [("f16x3", 0), ("f16x3", 1), ("bf16x6", 1), ("fp32", 1)])
def test_poisoned_workspaces_change_nothing(dp, fusion):
    """Every activation workspace filled with NaN bytes (0xFF) or finite garbage (0x3C, which a ReLU does not swallow) before every pass:
    logits and split flags bit-identical to an unpoisoned run, the saturation flag down - for a ragged chunking (13 blocks, chunk 5), the
    fused entry point's own logit buffers (records, no logit pointers), and overlap mode on a 1024-block call."""
    from pmp_vvc_tip2023_amd import engine, synth
    y, u, v = _edge_blocks(n_random=1)
    y, u, v = np.concatenate([y, y[:1]]), np.concatenate([u, u[:1]]), np.concatenate([v, v[:1]])    # 13 blocks
    by, bu, bv = synth.recipe_r_blocks(1024, 31)
    by[:13], bu[:13], bv[:13] = y, u, v
    e = engine.Engine(0, allow_synthetic_mtt=True)
    try:
        e.set_precision(dp)
        e.set_fusion(fusion)
        e.set_saturation_policy("ignore")
        dev = torch.device("cuda:0")
        for comp in ("Luma", "Chroma"):
            ref = e.infer_postprocess(comp, 22, y, u, v, want_logits=True)
            big = e.infer_postprocess(comp, 22, by, bu, bv, want_logits=True) if comp == "Luma" else None
            d_y, d_u, d_v = (torch.from_numpy(a).to(dev) for a in (y, u, v))
            rec = torch.empty((13, 1344), dtype=torch.uint8, device=dev)
            for pattern in (1, 2):
                _poison(e, pattern)
                e.clear_saturation()
                got = e.infer_postprocess(comp, 22, y, u, v, want_logits=True)
                e.set_chunk(5)
                ragged = e.infer_postprocess(comp, 22, y, u, v, want_logits=True)
                e.set_chunk(4096)
                e.infer_postprocess_records_device(comp, 22, d_y.data_ptr(), d_u.data_ptr(), d_v.data_ptr(), 13, rec.data_ptr())
                e.synchronize()
                r = rec.cpu().numpy()
                if big is not None:
                    e.set_overlap(True)
                    ov = e.infer_postprocess(comp, 22, by, bu, bv, want_logits=True)
                    e.set_overlap(False)
                    assert all(np.array_equal(a, b) for a, b in zip(big, ov)), "%s %s poison %d: overlap mode differs" % (dp, comp, pattern)
                assert not e.saturated(), (dp, comp, pattern)
                _poison(e, 0)
                for nm, a, b, c in zip(("hor", "ver", "qt_u8", "dire_i8", "qt", "bt", "dire"), ref, got, ragged):
                    assert np.array_equal(a, b) and np.array_equal(a, c), "%s fusion %d %s poison %d: %s differs" % (dp, fusion, comp, pattern, nm)
                assert np.array_equal(r[:, :256].reshape(13, 16, 16), ref[0]) and np.array_equal(r[:, 576:].view(np.int8).reshape(13, 3, 16, 16), ref[3])
    finally:
        e.close()


def test_parked_poisoned_workspace_is_not_read(monkeypatch):
    """A context that takes over the parked workspace of a destroyed context whose workspace was poisoned computes what a fresh one does.
    The destroyed context ran other blocks and, last, a one-block pass behind a full 0xFF fill: the buffer it parks is NaN bytes but for
    that pass's few tensors.  The new context must really run in that buffer: it allocates no new workspace."""
    from pmp_vvc_tip2023_amd import engine, synth
    monkeypatch.delenv("PMP_PARK_WORKSPACE", raising=False)
    y, _, _ = synth.recipe_r_blocks(64, 12)
    y = np.concatenate([y] * 16)                             # 1024 blocks: 2.5 GB of workspace, above the parking threshold
    other, _, _ = synth.recipe_r_blocks(1024, 13)
    e = engine.Engine(0, allow_synthetic_mtt=True)
    try:
        e.lib.pmp_trim()                                     # nothing parked: this context allocates afresh
        e.set_saturation_policy("ignore")
        ref = e.infer_postprocess("Luma", 22, y, want_logits=True)
    finally:
        e.close()
    e.lib.pmp_trim()
    e = engine.Engine(0, allow_synthetic_mtt=True)
    try:
        e.set_saturation_policy("ignore")
        _poison(e, 1)
        e.infer_postprocess("Luma", 22, other, want_logits=True)
        e.infer_postprocess("Luma", 22, y[:1], want_logits=True)
    finally:
        e.close()                                            # parks the poisoned 2.5 GB workspace
    e = engine.Engine(0, allow_synthetic_mtt=True)
    try:
        e.set_saturation_policy("ignore")
        e.load("Luma", 22)
        torch.cuda.synchronize(0)
        free0 = torch.cuda.mem_get_info(0)[0]
        got = e.infer_postprocess("Luma", 22, y, want_logits=True)
        torch.cuda.synchronize(0)
        grew = free0 - torch.cuda.mem_get_info(0)[0]
        assert grew < 512 * 2 ** 20, "the context allocated %d MB instead of taking over the parked workspace" % (grew >> 20)
        assert not e.saturated()
    finally:
        e.close()
    e.lib.pmp_trim()
    for a, b in zip(ref, got):
        assert np.array_equal(a, b)


def _lifecycle_cycle(y):
    """One context's whole life on 16 blocks: a host-pointer call of every family, so that every staging buffer, the logits, the outputs
    and the workspaces exist, then taps.  -> (workspace_bytes() before close, the device's free bytes after close and pmp_trim)."""
    from pmp_vvc_tip2023_amd import engine
    n = y.shape[0]
    labels = np.zeros((n, 8, 8), np.uint8), np.zeros((n, 16, 16), np.uint8), np.zeros((n, 3, 16, 16), np.int8)   # unsplit blocks
    planes = np.zeros((1, 128, 128), np.uint8), np.zeros((1, 64, 64), np.uint8), np.zeros((1, 64, 64), np.uint8)
    e = engine.Engine(0, allow_synthetic_mtt=True)
    try:
        e.load("Luma", 22)
        qt, bt, dire = e.inference_pre_QBD("Luma", 22, y)
        e.infer_postprocess("Luma", 22, y)
        e.post_process(qt, bt, dire, "Luma")
        e.output_block_yuv(*planes)
        e.gen_seq_sub_map(*labels, True)
        e.label_partition(*labels, 1)
        e.val_stats(22, qt=qt, bt=bt, dire=dire, qt8=labels[0], msbt=np.zeros((n, 3, 16, 16), np.uint8), msdire=labels[2])
        _taps_on(e, True)
        e.infer_postprocess("Luma", 22, y)
        ws = e.workspace_bytes()
    finally:
        e.close()
    e.lib.pmp_trim()
    torch.cuda.synchronize(0)
    return ws, torch.cuda.mem_get_info(0)[0]


def test_context_lifecycle_leaks_nothing(monkeypatch):
    """Six contexts created, used through every entry point family and destroyed, with parking off and with parking on (and trimmed):
    the device's free memory after the sixth is not below that after the first by as much as one activation workspace - the smallest
    workspace_bytes() seen, so a workspace, a logit set or a tap set leaked per cycle shows within the five cycles between them.  Other
    processes on the card may move the numbers: the twelve cycles may run a second time, once.
    Two unmeasured cycles come first: in a fresh process free memory falls by 72 MB once, between the first context's end and the
    second's, and then stays where it is for every later cycle (profiles/ctx_lifecycle.txt): a one-time cost of the process, not a leak
    per context, and already paid when this test runs behind others."""
    from pmp_vvc_tip2023_amd import synth
    y, _, _ = synth.recipe_r_blocks(16, 5)
    for _ in range(2):
        _lifecycle_cycle(y)

    def twelve():
        lost = []
        for park in ("0", None):
            if park is None:
                monkeypatch.delenv("PMP_PARK_WORKSPACE", raising=False)
            else:
                monkeypatch.setenv("PMP_PARK_WORKSPACE", park)
            runs = [_lifecycle_cycle(y) for _ in range(6)]
            bound = min(ws for ws, _ in runs)
            print("\ncontext lifecycle, parking %s: workspace_bytes %s, free bytes after each cycle %s"
                  % ("off" if park else "on", sorted({ws for ws, _ in runs}), [f for _, f in runs]))
            assert bound > 0
            lost.append((runs[0][1] - runs[5][1], bound))
        return lost

    lost = twelve()
    if any(d >= bound for d, bound in lost):
        lost = twelve()
    for d, bound in lost:
        assert d < bound, "free memory fell by %d bytes over five context lifecycles (one workspace: %d)" % (d, bound)


# ------------------------------------------------------------------------------------------------ 4. block-order independence
@pytest.mark.parametrize("dp,comp", [("f16x3", "Luma"), ("f16x3", "Chroma"), ("fp32", "Luma")])
def test_block_order_does_not_matter(dp, comp):
    """n = 1031 (prime, above 2 x 256 CUs x 2 workgroups): the persistent kernels (chain16, rbfuse32, two workgroups per CU looping over
    blocks with LDS kept between them) run ragged final rounds.  A permuted batch gives the permuted outputs bit for bit, and eight
    sampled blocks run alone give their bits in the batch; all-0 and all-255 blocks sit next to busy ones."""
    from pmp_vvc_tip2023_amd import engine, synth
    n = 1031
    y, u, v = synth.recipe_r_blocks(n, 55)
    ey, eu, ev = _edge_blocks(n_random=0)
    for k in range(len(ey)):
        y[3 * k], u[3 * k], v[3 * k] = ey[k], eu[k], ev[k]
    rng = np.random.default_rng(8)
    perm = rng.permutation(n)
    e = engine.Engine(0, allow_synthetic_mtt=True)
    try:
        e.set_precision(dp)
        e.set_saturation_policy("ignore")
        a = e.inference_pre_QBD(comp, 22, y, u, v)
        b = e.inference_pre_QBD(comp, 22, y[perm], u[perm], v[perm])
        for p, q in zip(a, b):
            assert np.array_equal(p[perm], q)
        for i in sorted(rng.choice(n, 8, replace=False).tolist() + [0, 3]):
            s = e.inference_pre_QBD(comp, 22, y[i:i + 1], u[i:i + 1], v[i:i + 1])
            for p, q in zip(a, s):
                assert np.array_equal(p[i:i + 1], q), (dp, comp, i)
        assert not e.saturated()
    finally:
        e.close()


def test_taps_refuse_what_they_cannot_record():
    """Taps need one pass of at most 64 blocks without overlap mode (PMP_E_INVALID otherwise); off, they cost nothing and record nothing."""
    from pmp_vvc_tip2023_amd import engine, synth, _lib
    y, _, _ = synth.recipe_r_blocks(13, 3)
    e = engine.Engine(0, allow_synthetic_mtt=True)
    try:
        e.inference_pre_QBD("Luma", 22, y)
        assert _tap(e, "q/stem") is None
        _taps_on(e, True)
        e.set_chunk(5)
        with pytest.raises(_lib.PmpError) as ei:
            e.inference_pre_QBD("Luma", 22, y)
        assert ei.value.code == -1
        e.set_chunk(4096)
        with pytest.raises(_lib.PmpError):
            e.inference_pre_QBD("Luma", 22, np.concatenate([y] * 5))
        e.inference_pre_QBD("Luma", 22, y)
        t, cr = _tap(e, "q/stem")
        assert t.shape == (13, 32, 64, 64) and cr == 32
        assert _tap(e, "bd/trunk_M1.3")[0].shape == (13, 64, 64, 64)
        assert _tap(e, "q/no_such_tensor") is None
    finally:
        e.close()


def _g1_luma4():
    from conftest import golden
    return np.ascontiguousarray(golden("g1_qt.npz")["block_y"][:4])


def test_taps_are_those_of_the_first_run_not_of_the_rerun():
    """A call whose range flag fired is run again on the fp32 datapath: its logits are the fp32 datapath's, bit for bit, while its taps stay
    those of the f16x3 run that fired - what a context that ignores the flag records, bit for bit.  Set-up of test_f16x3_range_guard
    (tests/test_gpu_parity.py): the range-stress MTT weights with activation scales off."""
    from pmp_vvc_tip2023_amd import engine
    y, w = _g1_luma4(), range_stress_weights()

    def run(precision, policy):
        e = engine.Engine(0, allow_synthetic_mtt=True)
        try:
            e.set_precision(precision)
            e.set_saturation_policy(policy)
            e.load("Luma", 22)
            e.load_pretrain_model("Luma_MSBD", 22, w)
            e.set_activation_scales(False)
            _taps_on(e, True)
            logits = e.inference_pre_QBD("Luma", 22, y)
            taps = {n: t[0] for n, t in ((n, _tap(e, n)) for n in _all_names()) if t is not None}     # shaped by the tap's own dims
            return logits, taps, e.saturation_reruns()
        finally:
            e.close()
    la, ta, reruns = run("f16x3", "rerun")
    assert reruns == 1, "the range flag did not fire on these blocks: the test checks nothing"
    _, tb, _ = run("f16x3", "ignore")
    assert "q/stem" in tb and "bd/trunk_M1.3" in tb
    for name, t in tb.items():
        assert name in ta, name
        assert ta[name].shape == t.shape, (name, ta[name].shape, t.shape)
        assert np.array_equal(ta[name], t), "%s: the re-run was recorded" % name
    lf, _, _ = run("fp32", "rerun")
    for a, b in zip(la, lf):
        assert np.array_equal(a, b), "the re-run is not the fp32 datapath"


def test_calibration_leaves_no_taps():
    """A pair loaded under another datapath is calibrated inside its first f16x3 call (fp32 passes of 16 blocks, launch per layer): the
    call's taps are its own tensors only.  With fusion on q/resblock_q4 stays in LDS, so the call has no such tensor - not the calibration's."""
    import ctypes as C
    from pmp_vvc_tip2023_amd import _lib, engine
    y = _g1_luma4()
    e = engine.Engine(0, allow_synthetic_mtt=True)
    try:
        e.set_precision("fp32")
        e.load("Luma", 22)
        e.set_precision("f16x3")
        e.set_fusion(True)
        _taps_on(e, True)
        e.inference_pre_QBD("Luma", 22, y)
        assert _tap(e, "q/stem")[0].shape[0] == 4
        with pytest.raises(_lib.PmpError) as ei:
            e._ck(e.lib.pmp_debug_get_tap(e.h, b"q/resblock_q4", None, 0, (C.c_int * 4)(), None))
        assert ei.value.code == -1          # PMP_E_INVALID
    finally:
        e.close()
