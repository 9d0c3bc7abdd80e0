"""ORACLE (test infrastructure, not product): a seeded table of ResidualBlock cases beyond the nets' shapes, and the table of the
convolution kernel instantiations the product library compiles.

tests/test_gpu_conv_sweep.py runs every case through pmp_debug_run_resblock (include/pmp.h: the loader's packing, the graph's conversion,
dispatch, exponent composition, in-place store and fused-kernel routing) and checks .t and the output against oracle/layers64.py per
element.  The cases span what the kernels accept rather than what the four nets use: N, non-square maps, odd K-group counts (the unpaired
K order of pack_h2), every Cout, 1x1 shortcuts of every width (Csc = 32 with Cout = 64 is the LDS shortcut form), gate, pool, fp32 output
and segment exponents - and the weight and activation edges of the f16x3 format: tensors whose max |w| gives a negative scale exponent or
hits the cap of 24, dead output channels (per-channel spreads of 2^8 .. 2^20), shortcut weights 2^+-12 / 2^+-18 away from the second
convolution they share a scale with, all-zero tensors, exact powers of two at the frexp edges of h2_scale_exp, activations that live only on
the border (a missing halo tap shows), negative inputs and values over 2^-20 .. 2^8.

tests/test_conv_cases_cpu.py checks INSTANTIATIONS against the kernel symbols of the built library and the table's reach (expected_kernels)."""
import math

import numpy as np

from oracle.layers64 import h2_scale_exp

DATAPATHS = ("f16x3", "bf16x6", "fp32")
PRECISION = {"fp32": 0, "bf16x6": 1, "f16x3": 2}

# Every conv_h2 / conv_x6 / conv_mfma kernel instantiation in libpmp_hip.so, by the name the launchers report (template arguments as
# integers): None = reached by the case table (expected_kernels says by which cases), a string = why nothing can reach it.
# conv_h2_kernel<KH, KW, NT, SC, LEAN>: NT = Cout / 16; SC 0 no shortcut source, 1 a 1x1 shortcut pass, 2 the 32-channel LDS shortcut.
INSTANTIATIONS = {}
for _k in (1, 3, 5):
    for _nt in (1, 2, 4):
        INSTANTIATIONS["conv_x6_kernel<%d,%d,%d>" % (_k, _k, _nt)] = None
        INSTANTIATIONS["conv_mfma_kernel<%d,%d,%d,%s>" % (_k, _k, _nt, "0,1" if _k == 1 else "2,2")] = None
        for _sc in (0, 1):
            if not (_k > 1 and _nt == 4 and _sc == 0):
                INSTANTIATIONS["conv_h2_kernel<%d,%d,%d,%d,0>" % (_k, _k, _nt, _sc)] = None
    if _k > 1:
        INSTANTIATIONS["conv_h2_kernel<%d,%d,4,0,1>" % (_k, _k)] = None     # Cout 64 without a shortcut source: the lean form
        INSTANTIATIONS["conv_h2_kernel<%d,%d,4,2,0>" % (_k, _k)] = None     # Cout 64, Csc 32
# rbfuse32_kernel<cin groups, cout groups, pool> (the fused 32x32 blocks, f16x3 with fusion on) are reported too; the hook reaches two
# of its three forms (the pooled one needs a block with a 1x1 shortcut from 16 to at most 16 channels, e.g. trunk_B3.2's 16 -> 8; this
# table's blocks have Cout in 16, 32, 64).
FUSED = ("rbfuse32_kernel<2,1,0>", "rbfuse32_kernel<1,2,0>")


def rb_scale_exps(w0, w2, wsc):
    """(k0, k2) as load_rb packs them: the second convolution and the 1x1 shortcut share one scale, min(k2, ksc)."""
    k2 = h2_scale_exp(w2)
    if wsc is not None:
        k2 = min(k2, h2_scale_exp(wsc))
    return h2_scale_exp(w0), k2


def fused32(c, fusion=True):
    """nets.cpp Graph::fused32 for a case of this table (the input reaches the block split, and the block consumes it)."""
    return (c["dp"] == "f16x3" and fusion and c["h"] == 32 and c["w"] == 32 and c["k"] == 3 and c["cin"] != c["cout"] and not c["gate"]
            and ((c["cin"] == 32 and c["cout"] == 16 and not c["pool"]) or (c["cin"] == 16 and c["cout"] == 32 and not c["pool"]))
            and not c["out_f32"])


def _one(dp, k, cout, sc, lean=False):
    nt = cout // 16
    if dp == "fp32":
        return "conv_mfma_kernel<%d,%d,%d,%s>" % (k, k, nt, "0,1" if k == 1 else "2,2")
    if dp == "bf16x6":
        return "conv_x6_kernel<%d,%d,%d>" % (k, k, nt)
    if k > 1 and nt == 4:
        return "conv_h2_kernel<%d,%d,4,%s>" % (k, k, {0: "0,1", 1: "1,0", 2: "2,0"}[sc])
    return "conv_h2_kernel<%d,%d,%d,%d,0>" % (k, k, nt, min(sc, 1))


def expected_kernels(c, fusion=True):
    """The instantiations, in launch order, that the product's dispatch picks for case c (launch_h2 / launch_x6 / launch_conv_mfma)."""
    if fused32(c, fusion):
        return ["rbfuse32_kernel<%d,%d,0>" % (c["cin"] // 16, c["cout"] // 16)]
    sc = 0 if c["cin"] == c["cout"] else (2 if c["cin"] == 32 else 1)
    return [_one(c["dp"], c["k"], c["cout"], 0), _one(c["dp"], c["k"], c["cout"], sc)]


def macs(c):
    return c["n"] * c["h"] * c["w"] * c["cout"] * ((c["cin"] + c["cout"]) * c["k"] ** 2 + (c["cin"] if c["cin"] != c["cout"] else 0))


# weight distributions: (gain of w0, gain of w2, gain of wsc relative to w2, per-output-channel spread (log2), values)
WDISTS = {
    "randn": (1.0, 1.0, 1.0, 0, "randn"),
    "w0_big": ("big", 1.0, 1.0, 0, "randn"),          # max |w0| >= 8192: a negative scale exponent
    "w2_big": (1.0, "big", 1.0, 0, "randn"),
    "cap": (2.0 ** -30, 2.0 ** -28, 1.0, 0, "randn"),  # max |w| far below 2^-11: k hits the cap of 24
    "dead8": (1.0, 1.0, 1.0, 8, "randn"),             # output channels spread over 2^8 / 2^16 / 2^20: dead channels of trained nets
    "dead16": (1.0, 1.0, 1.0, 16, "randn"),
    "dead20": (1.0, 1.0, 1.0, 20, "randn"),
    "sc+12": (1.0, 1.0, 2.0 ** 12, 0, "randn"),       # the shortcut sets the shared scale: w2 sits 2^12 / 2^18 below it
    "sc+18": (1.0, 1.0, 2.0 ** 18, 0, "randn"),
    "sc-12": (1.0, 1.0, 2.0 ** -12, 0, "randn"),      # w2 sets it: the shortcut sits below
    "sc-18": (1.0, 1.0, 2.0 ** -18, 0, "randn"),
    "zero_w0": (0.0, 1.0, 1.0, 0, "randn"),
    "zero_w2": (1.0, 0.0, 1.0, 0, "randn"),
    "pow2": (1.0, 1.0, 1.0, 0, "pow2"),               # exact powers of two, max |w| = 2^m: S * max = 4096, the lower frexp edge
    "edge8192": (1.0, 1.0, 1.0, 0, "edge8192"),       # max |w| = 8192 exactly and 8192 (1 - 2^-24): both sides of k = -1 / 0
}
XDISTS = ("spread", "signed", "border", "zero", "pow2", "wide")


def _weights(rng, cout, cin, k, gain, spread, kind):
    fan = cin * k * k
    w = rng.standard_normal((cout, cin, k, k)) / math.sqrt(fan)
    if kind == "pow2":
        w = np.sign(w) * np.exp2(np.round(np.log2(np.abs(w) + 1e-30)))
    if spread:
        w = w * np.exp2(-spread * np.arange(cout) / max(cout - 1, 1))[:, None, None, None]
    if gain == "big":
        w = w * (12288.0 / np.abs(w).max())
    else:
        w = w * gain
    if kind == "edge8192" and np.abs(w).max() > 0:
        w = w * (8192.0 / np.abs(w).max())
        w.flat[1 % w.size] = np.float32(8192.0 * (1 - 2.0 ** -24)) * np.sign(w.flat[1 % w.size] or 1)
    return w.astype(np.float32)


def _activation(rng, shape, kind, xmax):
    n, c, h, w = shape
    if kind == "zero":
        return np.zeros(shape, np.float32)
    mag = np.exp2(rng.uniform(-20, 0, shape)) * xmax
    if kind == "wide":        # log-uniform over 2^-20 .. 2^8 of the block's range, a quarter zero
        x = mag * (rng.random(shape) > 0.25)
    elif kind == "pow2":
        x = np.exp2(np.round(np.log2(mag))) * (rng.random(shape) > 0.25)
    elif kind == "signed":    # negative inputs (the attention inputs are signed logits)
        x = np.clip(rng.standard_normal(shape) / 4, -1, 1) * xmax
    elif kind == "border":    # non-zero only on the two outermost rows and columns: every halo tap of the edge tiles matters
        x = rng.random(shape) * xmax
        inner = np.ones((h, w), bool)
        inner[:2, :] = inner[-2:, :] = inner[:, :2] = inner[:, -2:] = False
        x[:, :, inner] = 0
    else:                     # spread: a post-ReLU activation, 2^-6 .. 2^6 of xmax / 64, a quarter zero
        x = np.exp2(rng.uniform(-12, 0, shape)) * xmax * (rng.random(shape) > 0.25)
    return x.astype(np.float32)


def tensors(c):
    """-> (x, w0, w2, wsc or None, gate or None) as float32 arrays for case c (deterministic in its seed)."""
    rng = np.random.default_rng(c["seed"])
    g0, g2, gsc, spread, kind = WDISTS[c["wdist"]]
    cin, cout, k = c["cin"], c["cout"], c["k"]
    w0 = _weights(rng, cout, cin, k, g0, spread, kind)
    kind2 = "randn" if kind == "edge8192" else kind          # the frexp edge on w0 alone: the block keeps a usable input range
    w2 = _weights(rng, cout, cout, k, g2, spread, kind2)
    wsc = None
    if cin != cout:
        wsc = _weights(rng, cout, cin, 1, 1.0, spread, kind2)
        wsc = (wsc * (gsc * (np.abs(w2).max() / max(float(np.abs(wsc).max()), 1e-30)) if g2 != 0 else wsc * gsc)).astype(np.float32)
    # keep every stored value well inside fp16 (the flag must stay clear): the input's range shrinks by the block's largest gain
    l1 = lambda w: float(np.abs(w).reshape(w.shape[0], -1).sum(1).max()) if w is not None else 0.0   # noqa: E731
    gain = max(1.0, l1(w0), l1(w0) * l1(w2), l1(w2), l1(wsc))
    xmax = min(2.0 ** 8, 2.0 ** 13 / gain) * 2.0 ** c["exp_x"]
    x = _activation(rng, (c["n"], cin, c["h"], c["w"]), c["xdist"], xmax)
    gate = None
    if c["gate"]:
        gate = (rng.random((c["n"], cout, c["h"], c["w"])) * 2.0 * 2.0 ** c["exp_gate"]).astype(np.float32)
    return x, w0, w2, wsc, gate


def _case(rng, dp, i, **kw):
    c = dict(dp=dp, n=1, h=16, w=16, cin=16, cout=16, k=3, gate=False, pool=False, out_f32=False, exp_x=0, exp_gate=0, exp_out=0,
             wdist="randn", xdist="spread")
    c.update(kw)
    if c["gate"]:
        c["pool"] = False
    if dp != "f16x3":
        c["exp_x"] = c["exp_gate"] = c["exp_out"] = 0
    elif not c["gate"]:
        c["exp_out"] = c["exp_x"]          # an ungated output stays in the input's segment (nets.cpp)
    elif c["cin"] == c["cout"]:
        c["exp_out"] = c["exp_x"] + c["exp_gate"]      # a gated identity block across a scale step is refused (nets.cpp Graph::rb)
    else:
        c["exp_out"] = c["exp_x"] + c["exp_gate"] + c["exp_out"] % 4     # x * gate stored at or below 2^14 of its scale
    c["seed"] = int(rng.integers(1 << 31)) ^ i
    c["id"] = "%s-%03d-n%d-%dx%d-%d-%d-k%d%s%s%s-%s-%s" % (dp, i, c["n"], c["h"], c["w"], c["cin"], c["cout"], c["k"],
                                                          "-gate" if c["gate"] else "", "-pool" if c["pool"] else "",
                                                          "-f32" if c["out_f32"] else "", c["wdist"], c["xdist"])
    return c


MAPS = [(16, 16), (32, 32), (64, 64), (16, 64), (64, 16), (48, 32)]
CINS = [16, 32, 48, 80, 128]
MAC_CAP = 2.0e9          # per case (float64 reference cost on the host)


def cases(seed=20261016):
    """The table: a systematic part (every instantiation on every datapath with every epilogue, every weight and activation edge on f16x3)
    and a seeded random part over the whole space; ~330 cases, their float64 references ~100 G multiply-adds."""
    rng = np.random.default_rng(seed)
    out = []

    def add(dp, **kw):
        c = _case(rng, dp, len(out), **kw)
        if macs(c) <= MAC_CAP:
            out.append(c)

    # 1) dispatch x epilogue on every datapath: k x Cout x shortcut width, cycling through the maps and epilogues
    j = 0
    for dp in DATAPATHS:
        for k in (1, 3, 5):
            for cout in (16, 32, 64):
                for cin in sorted({cout, 16, 32, 64, 128}):
                    h, w = MAPS[j % len(MAPS)]
                    ep = j % 4
                    add(dp, k=k, cout=cout, cin=cin, h=h, w=w, n=(1, 2, 5)[j % 3] if h * w <= 1024 else 1,
                        gate=ep == 1, pool=ep == 2, out_f32=ep == 3 or (ep == 2 and j % 8 == 6),
                        exp_x=(0, 3, -4, 6)[j % 4], exp_gate=(0, -2, 1)[j % 3], exp_out=(0, 2, -3, 5)[j % 4], xdist=XDISTS[j % 5])
                    j += 1
    # 2) the fused 32x32 forms and their launch-per-layer twins (run both ways by the test)
    for cin, cout in ((32, 16), (16, 32)):
        for xd in ("spread", "border", "signed"):
            add("f16x3", n=(1, 2, 5)[len(out) % 3], h=32, w=32, cin=cin, cout=cout, k=3, exp_x=(0, 2, -3)[len(out) % 3], xdist=xd)
    # 3) weight and activation edges on f16x3 (and a share on the exact datapaths)
    for wd in WDISTS:
        for r in range(6):
            dp = "f16x3" if r < 4 else DATAPATHS[1 + r % 2]
            k, cout = (3, 5, 1)[r % 3], (64, 32, 16)[r % 3]
            cin = (cout, 32, 16, 128, 48, 80)[r] if wd.startswith("sc") is False else (32, 16, 128, 48, 80, 64)[r]
            if cin == cout and wd.startswith("sc"):
                cin = 16 if cout != 16 else 32
            h, w = MAPS[(r + len(wd)) % len(MAPS)]
            add(dp, k=k, cout=cout, cin=cin, h=h, w=w, n=1 + r % 2, gate=r == 2, pool=r == 3, out_f32=r == 5,
                exp_x=(0, -5, 4, 2, 0, 0)[r], exp_gate=-1, exp_out=(0, 0, 3, 0, 0, 0)[r], wdist=wd, xdist=XDISTS[r % len(XDISTS)])
    # 4) seeded random fill over the whole space
    while len(out) < 330:
        dp = DATAPATHS[int(rng.integers(0, 5)) % 3 if rng.random() < 0.6 else 0]
        h, w = MAPS[int(rng.integers(len(MAPS)))]
        gate = rng.random() < 0.2
        add(dp, n=int(rng.choice([1, 2, 5])), h=h, w=w, cin=int(rng.choice(CINS)), cout=int(rng.choice([16, 32, 64])),
            k=int(rng.choice([1, 3, 3, 5, 5])), gate=gate, pool=not gate and rng.random() < 0.25, out_f32=rng.random() < 0.2,
            exp_x=int(rng.integers(-6, 7)), exp_gate=int(rng.integers(-3, 4)), exp_out=int(rng.integers(-6, 7)),
            wdist=str(rng.choice(list(WDISTS))), xdist=str(rng.choice(XDISTS)))
    return out


# shapes the kernels do not support: pmp_debug_run_resblock answers PMP_E_INVALID before any launch
REFUSED = [dict(n=1, h=16, w=16, cin=16, cout=48, k=3), dict(n=1, h=16, w=16, cin=16, cout=16, k=7),
           dict(n=1, h=24, w=16, cin=16, cout=16, k=3), dict(n=1, h=16, w=40, cin=16, cout=16, k=3),
           dict(n=1, h=16, w=16, cin=24, cout=16, k=3), dict(n=1, h=16, w=16, cin=16, cout=16, k=3, gate=1, pool=1),
           dict(n=0, h=16, w=16, cin=16, cout=16, k=3), dict(n=1, h=16, w=16, cin=16, cout=128, k=3)]
