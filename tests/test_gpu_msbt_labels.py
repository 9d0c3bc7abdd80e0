"""GPU: GenMSBtMap labels (include/pmp.h: pmp_msbt_labels) bit-exact with the reference-made G11 (tests/golden/g11_msbt.npz; inputs
rebuilt by tests/msbt_cases.py), the status bits where the reference has no answer (against the numpy restatement), the leaf budget
on worst-case blocks inside a time bound, every entry point, and gen_labels end to end on a synthesized dump directory."""
import os
import time

import numpy as np
import pytest

from conftest import golden
import gpu_rig
import msbt_cases as K

pytestmark = pytest.mark.gpu

WORST_BATCH_BOUND_S = 1.0       # a 1024-block launch of worst-case blocks (profiles/msbt_labels.txt)

eng = gpu_rig.engine_fixture()


@pytest.fixture(scope="module")
def g11():
    return golden("g11_msbt.npz")


def run(e, cf, qt, bt, dire):
    return e.gen_seq_sub_map(qt, bt, dire, is_luma=(cf == 1), return_status=True)


def expected(g11, name, cf, qt, bt, dire):
    """The reference's labels where it finished (status 0 or 2), the restatement's where it raised or the budget cuts."""
    m, st = K.restate_batch(qt, bt, dire, cf)
    ref, raised = g11[name + "_msbt"], g11[name + "_raised"]
    fin = ~raised & (st & K.OVER_BUDGET == 0)
    m[fin] = ref[fin]
    return m, st


@pytest.mark.parametrize("name", ["valid_cf1", "valid_cf2", "noisy", "ties", "ties_cf2", "qtdeep", "bigtree_cf1", "bigtree_cf2",
                                  "overbudget", "wrap"])
def test_kernel_equals_reference(eng, g11, name):
    cf, (qt, bt, dire) = [(c, x) for n, c, x in K.label_sets() if n == name][0]
    m, st = run(eng, cf, qt, bt, dire)
    em, est = expected(g11, name, cf, qt, bt, dire)
    assert np.array_equal(st, est), (name, np.nonzero(st != est))
    assert np.array_equal(m, em), (name, np.nonzero(np.any(m != em, axis=(1, 2, 3))))
    raised = g11[name + "_raised"]
    assert np.all(st[raised] & K.INCONSISTENT) and np.all(st[~raised] & K.INCONSISTENT == 0)
    if name.startswith("valid"):
        assert not st.any() and not raised.any()
        # synth's per-layer maps are an independent truth for valid partitions
        from pmp_vvc_tip2023_amd import synth
        rng = np.random.default_rng(K.SEEDS[name])
        truth = np.stack([synth.random_partition_maps(rng, cf)[1] for _ in range(len(qt))]).astype(np.uint8)
        assert np.array_equal(m, truth)
    if name == "qtdeep":
        assert np.all(st & K.QT_DEEP)
    if name == "overbudget":
        assert np.all(st & K.OVER_BUDGET)
    if name == "wrap":
        idx = g11["wrap_idx"]
        assert len(idx) and np.array_equal(m[idx][~raised[idx]], g11["wrap_msbt"][idx][~raised[idx]])


def test_worst_case_hits_budget_within_bound(eng):
    import torch
    for cf in (1, 2):
        qt, bt, dire = K.worst_blocks(1024)
        em, est = K.restate(qt[0], bt[0], dire[0], cf)
        d = [torch.from_numpy(a).cuda() for a in (qt, bt, dire)]
        out = torch.empty((1024, 3, 16, 16), dtype=torch.uint8, device="cuda"); st = torch.empty(1024, dtype=torch.uint8, device="cuda")
        eng.set_stream(torch.cuda.current_stream().cuda_stream)
        try:
            eng.msbt_labels_device(cf, d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), 1024, out.data_ptr(), st.data_ptr())  # warm-up
            torch.cuda.synchronize()
            t = time.perf_counter()
            eng.msbt_labels_device(cf, d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), 1024, out.data_ptr(), st.data_ptr())
            torch.cuda.synchronize()
            dt = time.perf_counter() - t
        finally:
            eng.set_stream(None)
        print("worst-case 1024 blocks cf %d: %.1f ms" % (cf, dt * 1e3))
        assert dt < WORST_BATCH_BOUND_S
        m, s = out.cpu().numpy(), st.cpu().numpy()
        assert np.all(s == est) and (cf == 2 or est & K.OVER_BUDGET)
        assert np.all(m == em[None])


def test_host_device_chunks_and_empty(eng):
    import torch
    qt, bt, dire = K.noisy_blocks(150, K.SEEDS["noisy"] + 5)
    m0, s0 = run(eng, 1, qt, bt, dire)
    eng.set_chunk(7)                             # 150 blocks = 22 passes through the staging buffers
    try:
        m1, s1 = run(eng, 1, qt, bt, dire)
    finally:
        eng.set_chunk(4096)
    assert np.array_equal(m0, m1) and np.array_equal(s0, s1)
    d = [torch.from_numpy(a).cuda() for a in (qt, bt, dire)]
    out = torch.zeros((150, 3, 16, 16), dtype=torch.uint8, device="cuda"); st = torch.zeros(150, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    eng.msbt_labels_device(1, d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), 150, out.data_ptr(), st.data_ptr())
    eng.synchronize()
    assert np.array_equal(out.cpu().numpy(), m0) and np.array_equal(st.cpu().numpy(), s0)
    # n = 0: nothing to do, no buffers needed
    m, s = run(eng, 1, qt[:0], bt[:0], dire[:0])
    assert m.shape == (0, 3, 16, 16) and s.shape == (0,)
    eng.msbt_labels_device(2, 0, 0, 0, 0, 0, 0)
    # one block through getSubMap
    one, st1 = eng.getSubMap(qt[3], bt[3], dire[3], 1, return_status=True)
    assert np.array_equal(one, m0[3]) and st1 == s0[3]


def test_poisoned_staging_changes_nothing(eng):
    qt, bt, dire = K.valid_blocks(64, 77, 1)
    qt[::5, :4, :4] = 5                          # some regions left zero (bit 2): those bytes must be written too
    m0, s0 = run(eng, 1, qt, bt, dire)
    for pattern in (1, 2):
        eng._ck(eng.lib.pmp_debug_poison_workspace(eng.h, pattern))
        try:
            m, s = run(eng, 1, qt, bt, dire)
        finally:
            eng._ck(eng.lib.pmp_debug_poison_workspace(eng.h, 0))
        assert np.array_equal(m, m0) and np.array_equal(s, s0), pattern


def test_device_call_is_stream_ordered(eng):
    """Inputs copied asynchronously (pinned host -> device on torch's stream) right before the call: the kernel sees them."""
    import torch
    qt, bt, dire = K.valid_blocks(2048, 91, 2)
    m0, s0 = run(eng, 2, qt, bt, dire)
    h = [torch.from_numpy(a).pin_memory() for a in (qt, bt, dire)]
    d = [torch.empty(a.shape, dtype=a.dtype, device="cuda") for a in h]
    out = torch.empty((2048, 3, 16, 16), dtype=torch.uint8, device="cuda"); st = torch.empty(2048, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()                 # a real stream: a null handle would hand the library back its own one
    eng.set_stream(stream.cuda_stream)
    try:
        with torch.cuda.stream(stream):
            for a, b in zip(d, h):
                a.copy_(b, non_blocking=True)
            eng.msbt_labels_device(2, d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), 2048, out.data_ptr(), st.data_ptr())
            m, s = out.cpu(), st.cpu()           # same stream: behind the kernel
    finally:
        eng.set_stream(None)
    assert np.array_equal(m.numpy(), m0) and np.array_equal(s.numpy(), s0)


def test_gen_labels_cli_equals_reference_pipeline(g11, tmp_path):
    from pmp_vvc_tip2023_amd import gen_labels
    table = K.write_pipe_dir(str(tmp_path / "dumps"))
    out = str(tmp_path / "out")
    rc = gen_labels.main(["--depthDir", str(tmp_path / "dumps"), "--seqTable", table, "--outDir", out,
                          "--qps", ",".join(str(q) for q in K.PIPE_QPS), "--ssRatio", str(K.PIPE_SS)])
    assert rc == 0
    for comp in ("Luma", "Chroma"):
        for qp in K.PIPE_QPS:
            key, stem = "pipe_%s_%d_" % (comp, qp), os.path.join(out, "Train_%s_QP%d_" % (comp, qp))
            for suffix, field, dt in (("QTdepth_Block8", "qt", np.uint8), ("BTdepth_Block16", "bt", np.uint8),
                                      ("MSdirection_Block16", "dire", np.int8), ("MSBTdepth_Block16", "msbt", np.uint8)):
                a = np.load(stem + suffix + ".npy")
                assert a.dtype == dt and np.array_equal(a, g11[key + field]), (comp, qp, suffix)
            assert not np.load(stem + "MSBTstatus.npy").any()
