"""GPU: Train_QBD's losses and their logit gradients (include/pmp.h: pmp_train_loss, logitstats.hip; pmp_vvc_tip2023_amd/train_loss.py).

Bounds.  The order of every addition is fixed by the header and the numpy restatement (tests/train_loss_cases.py) follows it, so sums,
loss and gradients are compared BIT FOR BIT (a NaN equals a NaN).  Against the reference's numbers (tests/golden/g14_train_loss.npz)
the bound is the distance its generator measured between the reference and that restatement (ref_vs_f64_loss, ref_vs_f64_grad): the
reference's own float32 rounding."""
import numpy as np
import pytest

from conftest import golden
import gpu_rig
import train_loss_cases as K
import val_cases as V

pytestmark = pytest.mark.gpu

ORDER = ("qt", "bt", "dire", "qt8", "msbt", "msdire")
GRADS = ("qt", "bt", "dire")

eng = gpu_rig.engine_fixture()


@pytest.fixture(scope="module")
def g14():
    return golden("g14_train_loss.npz")


def dev_call(e, comp, qp, kw, lam, grads=True, fill=None):
    """pmp_train_loss_device on uploaded copies -> (terms f64[13], loss, {gradients} or the untouched pre-filled buffers)."""
    import torch
    d = {k: torch.from_numpy(np.ascontiguousarray(kw[k])).cuda() if k in kw else None for k in ORDER}
    n = len(kw["qt"] if "qt" in kw else kw["bt"])
    out = torch.full((14,), -1.0, dtype=torch.float64, device="cuda")
    g = {k: torch.full(d[k].shape, float("nan"), device="cuda") for k in GRADS if d[k] is not None}
    if fill is not None:
        for t in g.values():
            t.view(torch.uint8).fill_(fill)
    torch.cuda.synchronize()
    P = lambda t: None if t is None else t.data_ptr()
    gp = [P(g.get(k)) if grads else None for k in GRADS]
    e.train_loss_device(comp, qp, *[P(d[k]) for k in ORDER], n, out.data_ptr(), out.data_ptr() + 104, *gp, params=lam)
    e.synchronize()
    torch.cuda.synchronize()
    o = out.cpu().numpy()
    return o[:13], float(o[13]), {k: t.cpu().numpy() for k, t in g.items()}


def want_of(c, mode, passes=None):
    kw, lam = K.kw_of(c, mode), K.lam_of(c, mode)
    T = K.terms(c["comp"], c["qp"], passes=passes, **kw)
    return T, K.loss_value(T, lam, c["n"]), K.grads(c["comp"], c["qp"], lam, c["n"], **kw)


def check_bits(what, got, want):
    T, loss, g = got
    wT, wloss, wg = want
    assert K.same_bits(np.asarray(T, np.float64), wT), (what, "terms", T, wT)
    assert K.same_bits(np.float64(loss).reshape(1), np.float64(wloss).reshape(1)), (what, "loss", loss, wloss)
    if g is not None:
        assert sorted(g) == sorted(wg), (what, sorted(g))
        for k in wg:
            assert g[k].dtype == np.float32 and K.same_bits(g[k].reshape(wg[k].shape), wg[k]), (what, "g_" + k, np.argwhere(g[k].reshape(wg[k].shape) != wg[k])[:4])


def check_reference(what, got, g14, name, mode):
    _, loss, g = got
    tol_l, tol_g = float(g14["ref_vs_f64_loss"]), float(g14["ref_vs_f64_grad"])
    d = V.rel_dist([float(g14["%s_%s_loss" % (name, mode)])], [loss])       # |ref - got| / |got|, as the generator measured it
    assert d <= tol_l, (what, d, tol_l)
    worst = 0.0
    for k, a in g.items():
        ref = g14["%s_%s_g_%s" % (name, mode, k)]
        a = a.reshape(ref.shape)
        assert K.same_zero_nan_pattern(ref, a), (what, k)
        dg = K.grad_dist(ref, a)
        assert dg <= tol_g, (what, k, dg, tol_g)
        worst = max(worst, dg)
    return d, worst


# ---- 1. every case, every form, host and device, against the restatement (bits) and the reference (its own rounding)
@pytest.mark.parametrize("name", list(K.CASES))
def test_every_case_equals_restatement_and_reference(eng, g14, name):
    c = K.make(name)
    for mode in K.MODES:
        kw, lam = K.kw_of(c, mode), K.lam_of(c, mode)
        want = want_of(c, mode)
        host = eng.train_loss(c["comp"], c["qp"], params=lam, **kw)
        dev = dev_call(eng, c["comp"], c["qp"], kw, lam)
        check_bits("host " + mode, host, want)
        check_bits("device " + mode, dev, want)
        for what, got in (("host", host), ("device", dev)):
            d, dg = check_reference("%s %s" % (what, mode), got, g14, name, mode)
            print("%s %s %s: vs the reference: loss %.3g, gradients %.3g" % (name, mode, what, d, dg))
        # value only: the same numbers, no gradients
        T, loss, g = eng.train_loss(c["comp"], c["qp"], params=lam, want_grads=False, **kw)
        assert g is None
        check_bits("host value-only " + mode, (T, loss, None), want)
        if c["comp"] == "Luma":                    # the luma matrix is the validation's: the same thirteen sums, bit for bit
            import torch
            d = {k: torch.from_numpy(np.ascontiguousarray(kw[k])).cuda() if k in kw else None for k in ORDER}
            S = torch.full((20,), -1.0, dtype=torch.float64, device="cuda")
            torch.cuda.synchronize()
            eng.val_stats_device(c["qp"], *[None if d[k] is None else d[k].data_ptr() for k in ORDER], c["n"], S.data_ptr())
            eng.synchronize()
            assert K.same_bits(S.cpu().numpy()[:13], np.asarray(dev[0], np.float64)), (name, mode, "terms differ from pmp_val_stats_device's")


# ---- 2. the same bits on every run, stream and chunk setting
def test_bits_do_not_depend_on_run_stream_or_chunk(eng):
    import torch
    c = K.make("luma30_n17")
    kw, lam = K.kw_of(c), K.lam_of(c, "qbd")
    a = dev_call(eng, c["comp"], c["qp"], kw, lam)
    b = dev_call(eng, c["comp"], c["qp"], kw, lam)
    check_bits("second run", b, a)
    s = torch.cuda.Stream()
    eng.set_stream(s.cuda_stream)
    try:
        with torch.cuda.stream(s):
            on_caller = dev_call(eng, c["comp"], c["qp"], kw, lam)
    finally:
        eng.set_stream(0)
    check_bits("caller's stream", on_caller, a)
    eng.set_chunk(4)
    try:
        chunked = dev_call(eng, c["comp"], c["qp"], kw, lam)
    finally:
        eng.set_chunk(4096)
    check_bits("device form at chunk 4", chunked, a)
    check_bits("restatement", a, want_of(c, "qbd"))


# ---- 3. the host form in passes: gradients of the whole call's n, sums in pass order
def test_host_form_passes(eng):
    c = K.make("chroma41_5_5_2")
    assert c["passes"] == (5, 5, 2) and c["n"] == 12
    for mode in K.MODES:
        kw, lam = K.kw_of(c, mode), K.lam_of(c, mode)
        one = eng.train_loss(c["comp"], c["qp"], params=lam, **kw)
        eng.set_chunk(5)
        try:
            three = eng.train_loss(c["comp"], c["qp"], params=lam, **kw)
        finally:
            eng.set_chunk(4096)
        check_bits("one pass " + mode, one, want_of(c, mode))
        check_bits("5 + 5 + 2 " + mode, three, want_of(c, mode, passes=c["passes"]))
        for k in one[2]:
            assert K.same_bits(one[2][k], three[2][k]), (mode, k)
    # a pass of its own is not a call of its own: blocks 0..4 as a call divide by 5, as a pass by 12
    alone = eng.train_loss(c["comp"], c["qp"], params=c["lam"], **K.kw_of(c, "qbd", slice(0, 5)))
    assert not np.array_equal(alone[2]["qt"], one[2]["qt"][:5])
    # value only through poisoned staging: the three gradient outputs are left out of every pass, the sums are the same bits
    eng.lib.pmp_debug_poison_workspace(eng.h, 1)
    eng.set_chunk(5)
    try:
        T, loss, g = eng.train_loss(c["comp"], c["qp"], params=c["lam"], want_grads=False, **K.kw_of(c))
    finally:
        eng.set_chunk(4096)
        eng.lib.pmp_debug_poison_workspace(eng.h, 0)
    assert g is None
    check_bits("value only, 5 + 5 + 2, poisoned", (T, loss, None), want_of(c, "qbd", passes=c["passes"]))


# ---- 4. every byte of a requested gradient is written; value only writes none
def test_gradient_buffers_overwritten_or_untouched(eng):
    c = K.make("chroma27_n3")
    for mode in K.MODES:
        kw, lam = K.kw_of(c, mode), K.lam_of(c, mode)
        want = want_of(c, mode)
        got = dev_call(eng, c["comp"], c["qp"], kw, lam, fill=0xFF)
        check_bits("pre-filled " + mode, got, want)
        T, loss, g = dev_call(eng, c["comp"], c["qp"], kw, lam, grads=False, fill=0xFF)
        check_bits("value only " + mode, (T, loss, None), want)
        for k, a in g.items():
            assert (a.view(np.uint8) == 0xFF).all(), (mode, k)
    eng.lib.pmp_debug_poison_workspace(eng.h, 1)          # the host form's staging buffers, poisoned before every pass
    try:
        check_bits("poisoned staging", eng.train_loss(c["comp"], c["qp"], params=c["lam"], **K.kw_of(c)), want_of(c, "qbd"))
    finally:
        eng.lib.pmp_debug_poison_workspace(eng.h, 0)


# ---- 5. n = 0 and everything that is PMP_E_INVALID, before any write
def test_empty_and_invalid(eng):
    import ctypes as C
    import torch
    from pmp_vvc_tip2023_amd import _lib, engine
    c = K.make("luma37_n3")
    n = c["n"]
    T, loss, g = eng.train_loss("Luma", 22, **K.kw_of(c, "qbd", slice(0, 0)))
    assert T.shape == (13,) and not T.any() and loss == 0.0 and g["qt"].shape == (0, 8, 8)
    out = torch.full((14,), 7.0, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    eng.train_loss_device("Chroma", 41, None, None, None, None, None, None, 0, out.data_ptr(), out.data_ptr() + 104)
    eng.synchronize()
    assert not out.cpu().numpy().any()

    d = {k: torch.from_numpy(np.ascontiguousarray(c[k])).cuda() for k in ORDER}
    g = {k: torch.full(d[k].shape, 3.0, device="cuda") for k in GRADS}
    out.fill_(7.0)
    torch.cuda.synchronize()
    P = lambda t: None if t is None else t.data_ptr()
    lp = engine.loss_params()

    def call(comp=0, qp=27, p=lp, ins=None, n_=n, terms=out.data_ptr(), loss=out.data_ptr() + 104, gr=None):
        ins = [P(d[k]) for k in ORDER] if ins is None else ins
        gr = [P(g[k]) for k in GRADS] if gr is None else gr
        return eng.lib.pmp_train_loss_device(eng.h, comp, qp, None if p is None else C.byref(p), *ins, n_, terms, loss, *gr)

    assert call() == 0                                                     # the valid call the others are variations of
    eng.synchronize()
    out.fill_(7.0)
    for t in g.values():
        t.fill_(3.0)
    torch.cuda.synchronize()
    I = [P(d[k]) for k in ORDER]
    G = [P(g[k]) for k in GRADS]
    bad_lam = engine.loss_params()
    bad_lam.lambd[1] = float("nan")
    inf_lam = engine.loss_params()
    inf_lam.lambq = float("inf")
    bad = {
        "comp": dict(comp=2), "qp 21": dict(qp=21), "qp 42": dict(qp=42), "n < 0": dict(n_=-1), "NaN weight": dict(p=bad_lam), "inf weight": dict(p=inf_lam),
        "null terms": dict(terms=None), "null loss": dict(loss=None),
        "logits without labels": dict(ins=[I[0], I[1], I[2], None, I[4], I[5]]), "bt without dire": dict(ins=[I[0], I[1], None, I[3], I[4], I[5]]),
        "nothing": dict(ins=[None] * 6, gr=[None] * 3),
        "g_qt missing": dict(gr=[None, G[1], G[2]]), "g_dire missing": dict(gr=[G[0], G[1], None]), "g_bt only": dict(gr=[None, G[1], None]),
        "g_qt in the MSBD form": dict(ins=[None, I[1], I[2], None, I[4], I[5]]), "g_bt in the Q form": dict(ins=[I[0], None, None, I[3], None, None]),
        "gradient aliases its logit": dict(gr=[G[0], I[1], G[2]]), "gradient overlaps an input": dict(gr=[G[0], G[1], I[2] + 16 * 4]),
        "bt misaligned": dict(ins=[I[0], I[1] + 4, I[2], I[3], I[4], I[5]]), "g_dire misaligned": dict(gr=[G[0], G[1], G[2] + 8]),
        "g_qt misaligned": dict(gr=[G[0] + 2, G[1], G[2]]), "terms misaligned": dict(terms=out.data_ptr() + 4),
    }
    for what, kw in bad.items():
        assert call(**kw) == -1, what
        assert b"pmp_train_loss" in eng.lib.pmp_last_error(eng.h), what
    eng.synchronize()
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == 7.0).all()
    for k, t in g.items():
        assert (t.cpu().numpy() == 3.0).all(), k
    for k in ORDER:                                                          # a refused alias wrote nothing into the inputs either
        assert np.array_equal(d[k].cpu().numpy(), c[k]), k
    # the host form refuses the same things
    T = np.full(13, 7.0); L = np.full(1, 7.0)
    q = np.ascontiguousarray(c["qt"]); q8 = np.ascontiguousarray(c["qt8"]); gq = np.full((n, 8, 8), 3.0, np.float32)
    H = lambda a: a.ctypes.data
    assert eng.lib.pmp_train_loss(eng.h, 0, 27, None, H(q), None, None, H(q8), None, None, n, H(T), H(L), H(q), None, None) == -1    # alias
    assert eng.lib.pmp_train_loss(eng.h, 0, 27, None, H(q), None, None, H(q8), None, None, n, H(T), H(L), H(gq), H(gq), None) == -1   # mix
    assert eng.lib.pmp_train_loss(eng.h, 0, 99, None, H(q), None, None, H(q8), None, None, n, H(T), H(L), H(gq), None, None) == -1
    assert (T == 7.0).all() and L[0] == 7.0 and (gq == 3.0).all() and np.array_equal(q, c["qt"])
    with pytest.raises(_lib.PmpError):
        eng.train_loss("Luma", 21, **K.kw_of(c))
    with pytest.raises(ValueError):
        eng.train_loss("Luma", 27, qt=c["qt"], qt8=None)


# ---- 6. the autograd wrapper
def test_autograd_wrapper(eng):
    import torch
    from pmp_vvc_tip2023_amd import train_loss
    c = K.make("chroma27_n3")
    n = c["n"]
    lam = c["lam"]
    want_T, want_loss, want_g = want_of(c, "qbd")
    lab = [torch.from_numpy(c[k]).cuda() for k in ("qt8", "msbt", "msdire")]
    assert lab[0].dtype == torch.uint8 and lab[1].dtype == torch.uint8 and lab[2].dtype == torch.int8

    def heads():
        qt = torch.from_numpy(c["qt"]).reshape(n, 1, 8, 8).cuda().requires_grad_()
        bd = [torch.stack([torch.from_numpy(c["bt"][:, k]), torch.from_numpy(c["dire"][:, k])], dim=1).cuda().requires_grad_() for k in range(3)]
        return qt, bd

    def head_grads(qt, bd):
        return {"qt": qt.grad.reshape(n, 8, 8).cpu().numpy(), "bt": np.stack([b.grad[:, 0].cpu().numpy() for b in bd], axis=1),
                "dire": np.stack([b.grad[:, 1].cpu().numpy() for b in bd], axis=1)}

    try:
        qt, bd = heads()
        loss, terms = train_loss.loss_func_QBD(eng, qt, bd[0], bd[1], bd[2], *lab, False, c["qp"], lam, return_terms=True)
        assert loss.dtype == torch.float32 and loss.dim() == 0 and loss.is_cuda and loss.requires_grad
        assert terms.dtype == torch.float64 and terms.shape == (13,) and terms.is_cuda and not terms.requires_grad
        loss.backward()
        assert loss.item() == np.float32(want_loss) and K.same_bits(terms.cpu().numpy(), want_T)
        g1 = head_grads(qt, bd)
        for k in GRADS:                                  # values: torch's own regrouping adds zeros, which may turn a -0.0 into +0.0
            assert np.array_equal(g1[k], want_g[k]), k
        qt, bd = heads()
        train_loss.loss_func_QBD(eng, qt, bd[0], bd[1], bd[2], *lab, False, c["qp"], lam).backward(torch.tensor(2.0, device="cuda"))
        g2 = head_grads(qt, bd)
        for k in GRADS:
            assert np.array_equal(g2[k], want_g[k] * np.float32(2)), k          # exactly twice
        # the MTT-only and QT-only forms; a loss scaled by the caller reaches the heads through grad_output
        qt, bd = heads()
        lm = train_loss.loss_func_MSBD(eng, bd[0], bd[1], bd[2], lab[1], lab[2], False, c["qp"], lam)
        lq = train_loss.l1_loss_Q(eng, qt, lab[0])
        (0.5 * lm + 4.0 * lq).backward()
        g3 = head_grads(qt, bd)
        wm, wq = want_of(c, "bd"), want_of(c, "q")
        assert lm.item() == np.float32(wm[1]) and lq.item() == np.float32(wq[1])
        assert np.array_equal(g3["bt"], wm[2]["bt"] * np.float32(0.5)) and np.array_equal(g3["dire"], wm[2]["dire"] * np.float32(0.5))
        assert np.array_equal(g3["qt"], wq[2]["qt"] * np.float32(4))
        # no gradient wanted: value only
        with torch.no_grad():
            qt, bd = heads()
            lv = train_loss.loss_func_QBD(eng, qt.detach(), bd[0].detach(), bd[1].detach(), bd[2].detach(), *lab, False, c["qp"], lam)
        assert not lv.requires_grad and lv.item() == np.float32(want_loss)
    finally:
        eng.set_stream(0)
