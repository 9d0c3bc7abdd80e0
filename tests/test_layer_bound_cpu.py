"""The float64 layer bound of oracle/layers64.py is neither vacuous nor violated by the documented arithmetic (no GPU needed).

float32-torch emulations of each datapath's convolution (the operand splits, the products the kernels form, fp32 accumulation, the
store format) must stay inside the bound at the nets' real shapes; each mutant - an arithmetic slip a kernel could make - must exceed it
by at least 16x.  A change that loosens C_DP, R_DP or FLOOR_DP far enough to hide one of these mutants fails here."""
import math

import pytest
import torch
import torch.nn.functional as F

from oracle import layers64 as L

# (kernel, cin, cout, 1x1 shortcut, pool): 3x3 64->64 and 5x5 64->64 identity blocks, 32->64 with shortcut, 16->32 with shortcut + pool
SHAPES = [(3, 64, 64, False, False), (5, 64, 64, False, False), (3, 32, 64, True, False), (3, 16, 32, True, True)]
# mutants per datapath: the ones every datapath could make, plus its own product set and scale (fp32 and bf16x6 have no out_scale)
_COMMON = ["store_fp16", "store_bf16", "border_tap", "last_k_group"]
MUTANTS = {"fp32": _COMMON, "bf16x6": _COMMON + ["five_products"],
           "f16x3": _COMMON + ["two_products_x0w", "two_products_xw0", "out_scale"]}


def _f16(a):
    return a.to(torch.float16).to(torch.float32)


def _bf16(a):
    return a.to(torch.bfloat16).to(torch.float32)


def _split2(a):
    h0 = _f16(a)
    return h0, _f16(a - h0)


def _split3(a):
    b0 = _bf16(a)
    b1 = _bf16(a - b0)
    return b0, b1, _bf16(a - b0 - b1)


def _scale_exp(w):
    """pack.cpp h2_scale_exp: S = 2^k puts max |S*w| in [4096, 8192), k capped to [-100, 24]."""
    return L.h2_scale_exp(w.numpy())


def _conv_seq(x, w, pad, group):
    """Convolution as the MFMA kernels accumulate it: a float32 running sum over the K products in K order, rounded once per `group`
    products - 1 for the fp32 MFMA (a k-ordered fmaf chain, cdna_hip_programming guide), 8 for the fp16 / bf16 MFMAs (groups of eight
    products added with guard bits and one rounding, EXPERIMENTS.md)."""
    n, _, h, wd = x.shape
    cols = F.unfold(x.double(), w.shape[2:], padding=pad)        # [n, cin*k*k, h*wd]
    wf = w.double().reshape(w.shape[0], -1)
    acc = torch.zeros((n, w.shape[0], h * wd), dtype=torch.float32)
    for j in range(0, wf.shape[1], group):
        part = torch.einsum("ok,nkl->nol", wf[:, j:j + group], cols[:, j:j + group])
        acc = (acc.double() + part).float()
    return acc.reshape(n, w.shape[0], h, wd)


def _conv_dp(x, w, dp, mutant=None, k=None):
    """float32 accumulation of the products datapath dp forms; x holds values of the datapath's activation format.  k: the f16x3 scale
    exponent the weights are packed with (default: their own; a 1x1 shortcut is packed with the second convolution's, load_rb)."""
    pad = w.shape[2] // 2
    if mutant == "last_k_group":      # the last 16-channel K group never enters the accumulator
        x = x.clone()
        x[:, -16:] = 0
    if mutant == "border_tap":        # the bottom-centre tap dropped for the top output row only (it reads row 1, inside the map)
        full = _conv_dp(x, w, dp, k=k)
        wm = w.clone()
        wm[:, :, -1, w.shape[3] // 2] = 0
        full[:, :, 0, :] = _conv_dp(x, wm, dp, k=k)[:, :, 0, :]
        return full
    if dp == "fp32":
        return _conv_seq(x, w, pad, 1)
    if dp == "bf16x6":
        a, b = _split3(x), _split3(w)
        pairs = [(0, 0), (0, 1), (1, 0), (0, 2), (1, 1), (2, 0)]
        if mutant == "five_products":     # x0 * w1 dropped
            pairs.remove((0, 1))
        return _conv_seq(torch.cat([a[i] for i, _ in pairs], 1), torch.cat([b[j] for _, j in pairs], 1), pad, 8)
    if k is None or mutant == "sc_own_scale":     # sc_own_scale: the shortcut packed with its own exponent, unpacked with the shared one
        k, k_out = _scale_exp(w), k
    else:
        k_out = k
    k_out = k if k_out is None else k_out
    x0, x1 = _split2(x)
    w0, w1 = _split2(w * 2.0 ** k)
    pairs = {"two_products_x0w": [(x0, w0), (x0, w1)], "two_products_xw0": [(x0, w0), (x1, w0)]}.get(mutant, [(x0, w0), (x0, w1), (x1, w0)])
    acc = _conv_seq(torch.cat([p for p, _ in pairs], 1), torch.cat([q for _, q in pairs], 1), pad, 8)
    return acc * 2.0 ** (-k_out + (1 if mutant == "out_scale" else 0))


def _store(v, dp, mutant=None):
    if mutant == "store_fp16":
        return _f16(v).double()
    if mutant == "store_bf16":
        return _bf16(v).double()
    if dp == "f16x3":
        h0, h1 = _split2(v)
        return h0.double() + h1.double()
    return v.double()       # fp32 and split-3 (exact for fp32 values)


def _activation(shape, g, dp):
    """A post-ReLU activation tensor of the datapath's format: non-negative, a quarter of it zero, spread over 2^-6..2^6."""
    x = torch.exp2(torch.empty(shape).uniform_(-6, 6, generator=g)) * (torch.rand(shape, generator=g) > 0.25)
    return _store(x, dp)


# weight distributions of the f16x3 edges (oracle/conv_cases.py WDISTS): (gain of w0, gain of w2, gain of wsc relative to w2, per-output-
# channel spread in powers of two)
WDISTS = {"randn": (1.0, 1.0, 1.0, 0), "dead20": (1.0, 1.0, 1.0, 20), "dead16": (1.0, 1.0, 1.0, 16), "sc+18": (1.0, 1.0, 2.0 ** 18, 0),
          "sc-18": (1.0, 1.0, 2.0 ** -18, 0), "sc-12": (1.0, 1.0, 2.0 ** -12, 0), "cap": (2.0 ** -30, 2.0 ** -28, 1.0, 0),
          "big": (2.0 ** 14, 2.0 ** -14, 1.0, 0)}


def _weights(g, cout, cin, k, gain, spread):
    w = torch.randn((cout, cin, k, k), generator=g) / math.sqrt(cin * k * k)
    if spread:
        w = w * torch.exp2(-spread * torch.arange(cout, dtype=torch.float32) / max(cout - 1, 1))[:, None, None, None]
    return (w * gain).float()


def _run(shape, dp, mutant=None, seed=0, wdist="randn", hw=(16, 16)):
    """Both launches of a ResidualBlock emulated; -> (max ratio of .t, max ratio of the output).  On f16x3 the 1x1 shortcut is packed
    with the second convolution's scale exponent, min(k(w2), k(wsc)), and shares its accumulator, as load_rb and the kernels do."""
    k, cin, cout, sc, pool = shape
    g0, g2, gsc, spread = WDISTS[wdist]
    g = torch.Generator().manual_seed(1000 * k + cin + seed)
    x = _activation((2, cin) + hw, g, dp)
    x = _store((x / max(1.0, g0, g0 * g2, gsc if sc else 1.0)).float(), dp)     # every stored value stays inside fp16
    w0 = _weights(g, cout, cin, k, g0, spread)
    w2 = _weights(g, cout, cout, k, g2, spread)
    wsc = _weights(g, cout, cin, 1, 1.0, spread) if sc else None
    if sc:
        wsc = (wsc * (gsc * float(w2.abs().max() / wsc.abs().max()))).float()
    t = _store(F.relu(_conv_dp(x.float(), w0, dp, mutant)), dp, mutant)
    t_ref, t_bnd = L.conv_t64(x, w0.double(), dp)
    k2 = min(_scale_exp(w2), _scale_exp(wsc)) if sc and dp == "f16x3" else None
    acc = _conv_dp(t.float(), w2, dp, None if mutant == "sc_own_scale" else mutant, k=k2)
    acc = acc + (_conv_dp(x.float(), wsc, dp, None if mutant == "border_tap" else mutant, k=k2) if sc else x.float())
    y = F.relu(acc)
    if pool:
        y = F.max_pool2d(y, 2)
    y = _store(y, dp, mutant)
    y_ref, y_bnd = L.conv_out64(x, t, w2.double(), wsc.double() if sc else None, dp, pool=pool)
    lt, ly = L.Layer("t", "", t_ref, t_bnd), L.Layer("y", "", y_ref, y_bnd)
    return L.ratio(t, lt), L.ratio(y, ly)


_IDS = lambda s: "%dx%d_%d_%d%s%s" % (s[0], s[0], s[1], s[2], "_sc" if s[3] else "", "_pool" if s[4] else "")   # noqa: E731


@pytest.mark.parametrize("dp", ["fp32", "bf16x6", "f16x3"])
@pytest.mark.parametrize("shape", SHAPES, ids=_IDS)
def test_documented_arithmetic_stays_inside_the_bound(shape, dp):
    """Inside the bound, and not loose by orders of magnitude: on every datapath the emulated error uses a good part of it (the
    accumulation term on fp32 and bf16x6, whose stores are exact; the split-2 store on f16x3), so loosening C_DP or R_DP fails here."""
    worst = 0.0
    for seed in range(2):
        rt, ry = _run(shape, dp, seed=seed)
        print("%s %s: max ratio .t %.3f, out %.3f" % (dp, shape, rt, ry))
        assert rt <= 1.0 and ry <= 1.0, (dp, shape, rt, ry)
        worst = max(worst, rt, ry)
    assert worst >= 1.0 / 8, (dp, shape, worst)


# the f16x3 edges beyond the nets' weights: dead channels, a shortcut far above / below the w2 it shares its scale with, the k = 24 cap, a
# tensor >= 8192 (negative k); on a 1x1-shortcut shape and a non-square pooled 5x5 one
EDGE_SHAPES = [((3, 32, 64, True, False), (16, 16)), ((5, 48, 16, True, True), (16, 48))]


@pytest.mark.parametrize("wdist", [w for w in WDISTS if w != "randn"])
@pytest.mark.parametrize("dp", ["fp32", "bf16x6", "f16x3"])
@pytest.mark.parametrize("shape,hw", EDGE_SHAPES, ids=["3x3_32_64_sc", "5x5_48_16_sc_pool_16x48"])
def test_weight_edges_stay_inside_the_bound(shape, hw, dp, wdist):
    rt, ry = _run(shape, dp, wdist=wdist, hw=hw)
    print("%s %s %s: max ratio .t %.3f, out %.3f" % (dp, wdist, shape, rt, ry))
    assert rt <= 1.0 and ry <= 1.0, (dp, wdist, shape, rt, ry)


# (not sc+18: there the second convolution adds 2^-18 of what the shortcut adds, so a slip in it is legitimately inside the output's bound)
@pytest.mark.parametrize("wdist", ["sc-12", "dead20", "big"])
@pytest.mark.parametrize("shape,hw", EDGE_SHAPES, ids=["3x3_32_64_sc", "5x5_48_16_sc_pool_16x48"])
def test_mutants_exceed_the_bound_at_the_weight_edges(shape, hw, wdist):
    """At the edges the bound gains a weight floor; a border tap, a last K group or an out_scale slip must still exceed it 16x, and so
    must a shortcut packed with its own exponent instead of the one it shares with w2 (the shortcut's products off by 2^(ksc - k2))."""
    for mutant in ("border_tap", "last_k_group", "out_scale") + (("sc_own_scale",) if wdist == "sc-12" else ()):
        rt, ry = _run(shape, "f16x3", mutant, wdist=wdist, hw=hw)
        print("f16x3 %s %s %s: max ratio .t %.1f, out %.1f" % (mutant, wdist, shape, rt, ry))
        assert ry >= 16 and (rt >= 16 or mutant == "sc_own_scale"), (mutant, wdist, shape, rt, ry)


def test_weight_floor_is_sharp():
    """W_FLOOR: weights 2^30 below their tensor's maximum keep an absolute error of half the subnormal fp16 step at the tensor's scale.
    Every weight of output channel 1 sits at 1.5 * 2^-24 / S, which rounds to 2^-23 / S (ties to even) with a zero low term: the error is
    2^-25 / S per weight, all of one sign, so the conv output misses by 2^-25 / S * sum|x|.  The bound must hold that and be met within 4x;
    without the floor it is exceeded by orders of magnitude."""
    g = torch.Generator().manual_seed(8)
    x = _store(torch.rand((2, 16, 16, 32), generator=g) * 1024 + 512, "f16x3")
    w = torch.randn((2, 16, 3, 3), generator=g)
    k = _scale_exp(w)
    w[1] = 1.5 * 2.0 ** (-24 - k)
    w = w.float()
    assert _scale_exp(w) == k
    got = _store(F.relu(_conv_dp(x.float(), w, "f16x3")), "f16x3")
    ref, bnd = L.conv_t64(x, w.double(), "f16x3")
    r = L.ratio(got[:, 1:], L.Layer("floor", "", ref[:, 1:], bnd[:, 1:]))
    assert 0.25 <= r <= 1.0, r
    no_floor = bnd[:, 1:] - L.wfloor(x, w.double(), "f16x3", k)
    assert L.ratio(got[:, 1:], L.Layer("floor", "", ref[:, 1:], no_floor)) >= 16


@pytest.mark.parametrize("mutant,dp", [(m, dp) for dp in ("fp32", "bf16x6", "f16x3") for m in MUTANTS[dp]])
@pytest.mark.parametrize("shape", SHAPES, ids=_IDS)
def test_mutants_exceed_the_bound_16x(shape, mutant, dp):
    rt, ry = _run(shape, dp, mutant)
    print("%s %s %s: max ratio .t %.1f, out %.1f" % (dp, mutant, shape, rt, ry))
    assert rt >= 16 and ry >= 16, (dp, mutant, shape, rt, ry)


def test_data_movement_bound_is_the_store_alone():
    """x6 / attention inputs: bit-exact on fp32 and bf16x6, one split-2 store on f16x3 - whose 2^-22 is met nearly with equality, so
    R_MOVE cannot be loosened unnoticed; a single fp16 store is far outside."""
    g = torch.Generator().manual_seed(5)
    v = torch.randn((2, 3, 32, 32), generator=g, dtype=torch.float64).float().double() * 100
    for dp in ("fp32", "bf16x6"):
        assert float(L._store_move(v, dp).max()) == 0.0
    lay = L.Layer("a", "data movement", v, L._store_move(v, "f16x3"))
    r = L.ratio(_store(v.float(), "f16x3"), lay)
    assert 0.25 <= r <= 1.0, r
    assert L.ratio(_f16(v.float()).double(), lay) >= 16


@pytest.mark.parametrize("dp", ["fp32", "bf16x6", "f16x3"])
def test_epilogue_and_store_term_is_sharp(dp):
    """R_DP alone, with no accumulation term: on fp32 and bf16x6 the epilogue rounds the accumulator + shortcut sum and the gate product
    in fp32 and stores exactly (split-3 holds fp32), two roundings of 2^-24; on f16x3 the split-2 store keeps 22 bits (its fp32 epilogue
    roundings sit far inside the accumulation term).  The bound must hold that and be met within 4x, so loosening R_DP fails here."""
    g = torch.Generator().manual_seed(7)
    # magnitudes 1..1024: the relative terms, not the split-2 floor (test_split2_floor_is_sharp), decide
    a, sc, gate = (torch.exp2(torch.empty((1 << 20,)).uniform_(0, 10, generator=g)) * torch.randn((1 << 20,), generator=g).sign()
                   for _ in range(3))
    if dp == "f16x3":
        ref = a.double()
        got = _store(a, dp)
    else:
        ref = (a.double() + sc.double()) * gate.double()
        got = ((a + sc) * gate).double()
    r = L.ratio(got, L.Layer("epilogue", "", ref, L.bound(torch.zeros_like(ref), ref, dp)))
    assert 0.25 <= r <= 1.0, (dp, r)


def test_split2_floor_is_sharp():
    """FLOOR_DP: values below fp16's normal range (2^-14) keep an absolute error of up to half the subnormal step, 2^-25, in a split-2
    store; the bound must hold it and be met within 4x (a looser floor fails), on the conv bound and on the data-movement bound alike."""
    g = torch.Generator().manual_seed(6)
    v = (torch.exp2(torch.empty((4, 16, 32, 32)).uniform_(-24, -12, generator=g)) * torch.rand((4, 16, 32, 32), generator=g)).double()
    v = v.float().double()
    stored = _store(v.float(), "f16x3")
    for bnd in (L._store_move(v, "f16x3"), L.bound(torch.zeros_like(v), v, "f16x3")):
        r = L.ratio(stored, L.Layer("tiny", "", v, bnd))
        assert 0.25 <= r <= 1.0, r


@pytest.mark.parametrize("comp", ["Luma", "Chroma"])
def test_layer_walk_reads_its_own_outputs(comp):
    """The launch-by-launch walk of both nets (oracle/layers64.py) fed with its own float64 results as 'taps': every launch's
    inputs exist under the names it reads, shapes chain up, and each layer reproduces itself exactly (ratio 0)."""
    from pmp_vvc_tip2023_amd import synth, weights as W
    luma = comp == "Luma"
    y, u, v = synth.recipe_r_blocks(2, 9)
    wq, _ = W.load_net_weights(comp + "_Q", 22)
    wb, _ = W.load_net_weights(comp + "_MSBD", 22, allow_synthetic=True)
    x = L.blocks64(luma, y, u, v)
    taps = {}
    names = []
    for gen in (L.q_layers(taps.__getitem__, wq, luma, x, "f16x3"), L.msbd_layers(taps.__getitem__, wb, luma, x, "f16x3")):
        for lay in gen:
            assert lay.ref.shape == lay.bound.shape and (lay.bound >= 0).all(), lay.name
            taps[lay.name] = lay.ref
            names.append(lay.name)
            assert L.ratio(lay.ref, lay) == 0.0
    assert len(names) == len(set(names)) == 67
    assert taps["q/head"].shape == (2, 1, 8, 8) and taps["bd/head2"].shape == (2, 2, 16, 16)
