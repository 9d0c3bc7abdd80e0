"""ORACLE (test infrastructure, not product): one launch of the four nets recomputed in float64, with an error bound.

tests/test_gpu_layers.py reads every intermediate tensor of a GPU inference call (pmp_debug_get_tap, include/pmp.h: the values the
consuming kernel reads, at true scale) and asks, launch by launch: given the GPU's own inputs to this launch, how far may its output be
from the exact result?  The answer follows the arithmetic each datapath documents (include/pmp.h, EXPERIMENTS.md precision study):

    |gpu - ref64| <= c_dp * 2^-24 * (|W| * |x|)  +  r_dp * |ref64|  +  floor_dp * 2^E

  (|W| * |x|)  the convolution of absolute values, shortcut (1x1 weights or the identity) and bias included: the sum of |products|
               that the accumulation rounds;
  c_dp         accumulation: fp32 MFMA is a k-ordered fmaf chain, 0.75-1.5e-7 * sum|a*b| against fp64 at K <= 1024 (1.3-2.5 units of
               2^-24); bf16x6 carries every operand as three bf16 terms (24 bits, exact for fp32 values) and drops the products below
               2^-24 relative, on top of the same fp32 accumulation; f16x3 carries the weights as two fp16 terms of S*w (a 2^-22 relative
               representation error) and drops the h1*h1' product (<= 2^-22 relative) on top of the fp32 accumulation;
  r_dp         rounding of the epilogue and the store: split-2 keeps 22 significand bits (2^-22; the fp32 epilogue roundings before
               it fall inside the c_dp term); fp32 and split-3 round the
               accumulator + shortcut sum and the gate product in fp32 (two roundings of 2^-24) and store exactly;
  floor_dp     the absolute floor of a split-2 store whose low term is subnormal in fp16 (half its 2^-24 ulp), in stored units:
               times 2^E of the tensor's segment (f16x3 activation scales) at true scale.
On f16x3 a convolution adds W_FLOOR * 2^-k * sum|x| (below): the absolute error of weights so far below their tensor's maximum that
their low fp16 term is subnormal (dead channels, a 1x1 shortcut that sets the scale it shares with w2; tests/test_gpu_conv_sweep.py).
ReLU and max-pool are 1-Lipschitz (the window maximum of the bound), a gate multiplies the bound by |gate|.  Pure data movement (the
multi-scale pool of the QT nets, the attention inputs) is exact up to the store: bit-exact on fp32 and bf16x6 (split-3 holds any fp32
value exactly), r_dp / floor_dp on f16x3.  The stems and the 8x8 direct blocks and heads run plain fp32 kernels except where noted.

MEASURED on an MI355X: a record of one run of tests/test_gpu_layers.py (which prints the table under `pytest -s` and asserts only that
every ratio is <= 1; real QT weights with uniform synthetic and trained-like MTT weights, Luma and Chroma, QP22 and QP37, 13 edge-case
blocks): the largest |gpu - ref64| / bound per layer class with the constants below.
    class           fp32 (c 24)   bf16x6 (c 32)   f16x3 (c 20)
    3x3 64->64      0.55          0.54            0.85 (store-bound)
    3x3             0.40          0.41            0.98 (store-bound; the 3x3 convs other than 64->64)
    5x5             0.53          0.44            0.50
    1x1 shortcut    0.36          0.46            0.93 (store-bound)
    stem            0.61          0.46            0.90 (logit-plane floor, below)
    direct 8x8      0.22          0.23            0.25 (fp32 kernel)
    head            0.43          0.42            0.44 (fp32 kernel)
    gate            0.26          0.24            1.00 (store-bound)
    pool            0.31          0.40            0.85 (store-bound)
    data movement   0 (bit-exact) 0 (bit-exact)   0.99 (store-bound)
"store-bound": the split-2 store's 2^-22 is met with equality by construction; the accumulation share is below 0.5 there.
The f16x3 MTT stem splits the raw QT logits into two fp16 terms itself, so its logit plane carries FLOOR_DP absolutely (msbd_layers).

Pinned fp32 behaviour of the nets stays in oracle/nets_torch.py; this module only reads its weight dicts.
"""
import math

import numpy as np
import torch
import torch.nn.functional as F

EPS = 2.0 ** -24

# c_dp: accumulation constant in units of 2^-24 * sum|products|, per datapath (see the module docstring for the model).  The model made
# executable - tests/test_layer_bound_cpu.py emulates each datapath's splits and its MFMA accumulation order (one rounding per product for
# fp32, per eight products for the fp16 / bf16 MFMAs) on activations spread over 2^-6..2^6 - reaches 9.0 (fp32), 13.4 (bf16x6: six products
# per term) and 10.1 (f16x3) units at the nets' shapes; c_dp is about twice that.  Largest ratio on the GPU: see tests/test_gpu_layers.py.
C_DP = {"fp32": 24.0, "bf16x6": 32.0, "f16x3": 20.0}
R_DP = {"fp32": 2.0 ** -23, "bf16x6": 2.0 ** -23, "f16x3": 2.0 ** -22}
FLOOR_DP = {"fp32": 0.0, "bf16x6": 0.0, "f16x3": 2.0 ** -25}
# data movement: what the store of an fp32 value in the datapath's activation format may change (split-3 holds fp32 exactly)
R_MOVE = {"fp32": 0.0, "bf16x6": 0.0, "f16x3": 2.0 ** -22}
# W_FLOOR: the absolute error of one f16x3 weight, in units of its tensor's scale S = 2^k (pack.cpp h2_scale_exp: max |S*w| in [4096, 8192)).
# pack_h2 stores S*w as h0 + h1, h0 = fp16(S*w), h1 = fp16(S*w - h0).  While h1 is a normal fp16 number its rounding is half an ulp of h1,
# at most 2^-11 * |S*w - h0| <= 2^-22 * |S*w| - the relative error that C_DP covers.  Once |S*w - h0| < 2^-14, h1 is subnormal (or h0 is,
# for |S*w| < 2^-14) and the rounding is half the subnormal step, 2^-25, whatever the weight: an ABSOLUTE error of 2^-25 * 2^-k per weight,
# and 2^-25 * 2^-k * sum|x| over the window of an output.  It overtakes the relative term for weights about 2^15 below their tensor's
# maximum: dead output channels of trained nets, and the second convolution of a block whose 1x1 shortcut sets the shared scale
# (weights_pack.cpp load_rb: k2 = min(k(w2), k(wsc))).  The dropped h1 * x1 product has no such floor: x1 is non-zero only for
# |x0| >= 2^-13, where it is within 2^-11 of x0's relative step.  tests/test_layer_bound_cpu.py::test_weight_floor_is_sharp.
W_FLOOR = {"fp32": 0.0, "bf16x6": 0.0, "f16x3": 2.0 ** -25}


def h2_scale_exp(w):
    """pack.cpp h2_scale_exp: S = 2^k with max |S*w| in [4096, 8192), k in [-100, 24]; 0 for an all-zero tensor."""
    m = float(np.abs(np.asarray(w, dtype=np.float32)).max()) if np.size(w) else 0.0
    if not m > 0 or not np.isfinite(m):
        return 0
    return int(min(24, max(-100, 13 - math.frexp(m)[1])))


def wfloor(x, w, dp, k):
    """W_FLOOR * 2^-k * sum|x| over each output's window (zero padding k//2), the same for every output channel."""
    if not W_FLOOR[dp]:
        return 0.0
    ks = w.shape[2]
    box = F.conv2d(x.abs().sum(1, keepdim=True), torch.ones((1, 1, ks, ks), dtype=x.dtype), padding=ks // 2)
    return W_FLOOR[dp] * 2.0 ** -k * box

def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64))


def _w(w, name):
    return _t(w[name])


def bound(acc_abs, ref, dp, E=0):
    """The bound of a conv output stored in datapath dp: accumulation term + store rounding + split-2 floor (E: segment exponent)."""
    return C_DP[dp] * EPS * acc_abs + R_DP[dp] * ref.abs() + FLOOR_DP[dp] * 2.0 ** E


def conv64(x, w, pad, bias=None):
    """float64 conv and its |W| * |x| companion."""
    y = F.conv2d(x, w, bias, padding=pad)
    a = F.conv2d(x.abs(), w.abs(), bias.abs() if bias is not None else None, padding=pad)
    return y, a


class Layer:
    """One launch recomputed: name of its output tap, layer class, float64 reference and bound (both [N,C,H,W] tensors)."""
    def __init__(self, name, cls, ref, bnd):
        self.name, self.cls, self.ref, self.bound = name, cls, ref, bnd


def conv_t64(x, w0, dp, E=0):
    """First launch of a ResidualBlock: relu(conv(x, w0)), pad k//2.  -> (ref, bound)."""
    pre, a = conv64(x, w0, w0.shape[2] // 2)
    t = F.relu(pre)
    return t, bound(a, t, dp, E) + wfloor(x, w0, dp, h2_scale_exp(w0))


def conv_out64(x, t, w2, wsc, dp, gate=None, pool=False, E=0):
    """Second launch: relu(conv(t, w2) + (conv1x1(x, wsc) or x)) [* gate] [-> 2x2 max-pool].  -> (ref, bound).  On f16x3 the 1x1
    shortcut shares the scale of w2 (weights_pack.cpp load_rb), and with it the weight floor."""
    pre, a = conv64(t, w2, w2.shape[2] // 2)
    k2 = h2_scale_exp(w2)
    if wsc is not None:
        s, sa = conv64(x, wsc, 0)
        k2 = min(k2, h2_scale_exp(wsc))
        fl = wfloor(t, w2, dp, k2) + wfloor(x, wsc, dp, k2)
    else:
        s, sa, fl = x, x.abs(), wfloor(t, w2, dp, k2)
    y, b = F.relu(pre + s), C_DP[dp] * EPS * (a + sa) + fl
    if gate is not None:
        y, b = y * gate, b * gate.abs()
    if pool:
        y, b = F.max_pool2d(y, 2), F.max_pool2d(b, 2)
    return y, b + R_DP[dp] * y.abs() + FLOOR_DP[dp] * 2.0 ** E


def rb_layers(get, w, net, name, dp, pool=False, gate=None, E=(0, 0)):
    """A ResidualBlock (Model_QBD.py:40-44) as its two launches: `.t` from the block input, the output from `.t` + the input (identity
    or 1x1 shortcut), then gate and 2x2 max-pool where the graph has them.  get(tap) -> float64 tensor [N,C_real,H,W] (the GPU's own
    inputs of each launch); E: segment exponents of .t and of the output."""
    x = get(net + "/" + _rb_input(net, name))
    w0, w2 = _w(w, name + ".left.0.weight"), _w(w, name + ".left.2.weight")
    scw = w.get(name + ".shortcut.0.weight")
    k = w0.shape[2]
    direct = x.shape[2] <= 8
    ldp = "fp32" if direct else dp            # the 8x8 layers run the plain fp32 direct kernel on every datapath
    tcls = "direct 8x8" if direct else ("3x3 64->64" if (k == 3 and w0.shape[0] == 64 and w0.shape[1] == 64) else "%dx%d" % (k, k))
    yield Layer(net + "/" + name + ".t", tcls, *conv_t64(x, w0, ldp, E[0]))
    g = get(net + "/" + gate) if gate is not None else None
    y, b = conv_out64(x, get(net + "/" + name + ".t"), w2, _t(scw) if scw is not None else None, ldp, g, pool, E[1])
    cls = ("direct 8x8" if direct else "gate" if gate is not None else "pool" if pool else
           "1x1 shortcut" if scw is not None else tcls)
    yield Layer(net + "/" + name, cls, y, b)


_Q_INPUT = {"resblock_q1": "stem", "resblock_q2": "resblock_q1", "resblock_q3": "resblock_q2", "resblock_q4": "x6",
            "resblock_q5": "resblock_q4", "resblock_q6": "resblock_q5"}


def _rb_input(net, name):
    if net == "q":
        return _Q_INPUT[name]
    trunk, i = name.rsplit(".", 1)
    i = int(i)
    if i > 0:
        return "%s.%d" % (trunk, i - 1)
    return {"trunk_M1": "stem", "trunk_M2": "trunk_M1.5", "trunk_B1": "trunk_M2.3", "trunk_Att1": "att_input1",
            "trunk_B2": "trunk_Att1.1", "trunk_Att2": "att_input2", "trunk_B3": "trunk_Att2.1"}[trunk]


def _store_move(ref, dp, E=0):
    return R_MOVE[dp] * ref.abs() + FLOOR_DP[dp] * (2.0 ** E if R_MOVE[dp] else 0.0)


def _up(a, s):
    return F.interpolate(a, scale_factor=s, mode="nearest")


def q_layers(get, wq, luma, blocks, dp):
    """Every launch of {Luma,Chroma}_Q_Net (Model_QBD.py:78-98) in launch order.  blocks: float64 [N,1,68,68] / [N,3,34,34] input."""
    p = 4 if luma else 2
    st, sa = conv64(F.pad(blocks, (0, p, 0, p)), _w(wq, "conv_q1.weight"), 0, _w(wq, "conv_q1.bias"))
    st = F.relu(st)
    yield Layer("q/stem", "stem", st, bound(sa, st, dp))
    yield from rb_layers(get, wq, "q", "resblock_q1", dp, pool=luma)
    yield from rb_layers(get, wq, "q", "resblock_q2", dp, pool=True)
    yield from rb_layers(get, wq, "q", "resblock_q3", dp)
    x5 = get("q/resblock_q3")
    x6 = torch.cat([x5] + [_up(F.max_pool2d(x5, s), s) for s in (2, 4, 8)], 1)
    yield Layer("q/x6", "data movement", x6, _store_move(x6, dp))
    yield from rb_layers(get, wq, "q", "resblock_q4", dp)
    yield from rb_layers(get, wq, "q", "resblock_q5", dp, pool=True)
    yield from rb_layers(get, wq, "q", "resblock_q6", dp)
    h, ha = conv64(get("q/resblock_q6"), _w(wq, "conv_q2.weight"), 1, _w(wq, "conv_q2.bias"))
    yield Layer("q/head", "head", h, bound(ha, h, "fp32"))


def msbd_layers(get, wb, luma, blocks, dp, exps=(0, 0, 0, 0, 0)):
    """Every launch of {Luma,Chroma}_MSBD_Net (Model_QBD.py:127-155) in launch order, from the GPU's own QT logits get("q/head") and
    heads get("bd/head<k>") = [bt[:,k], dire[:,k]].  exps: the f16x3 segment exponents (0 elsewhere)."""
    p, s = (4, 8) if luma else (2, 4)
    q = get("q/head")
    x2 = torch.cat([blocks, F.pad(_up(q, s), (p, 0, p, 0))], 1)
    outs = []
    for nm, pads in (("conv_b1_1", (0, p, 0, p)), ("conv_b1_2", (0, p, 0, 0)), ("conv_b1_3", (0, 0, 0, p))):
        outs.append(conv64(F.pad(x2, pads), _w(wb, nm + ".weight"), 0, _w(wb, nm + ".bias")))
    st = F.relu(torch.cat([o[0] for o in outs], 1))
    bnd = bound(torch.cat([o[1] for o in outs], 1), st, dp, exps[0])
    if FLOOR_DP[dp]:
        # f16x3: the stem splits the raw logits itself (two fp16 terms, conv_misc.hip stem_mfma_kernel): below |q| = 2^-2 the low term is
        # subnormal, an absolute floor of FLOOR_DP per logit, times the logit plane's |weights| (found by test_every_launch_within_its_
        # float64_bound on the all-zero chroma block, trained-like weights: 1.8e-7 on a stem output of 0.015, 2.2x the bound without it)
        mask = torch.zeros_like(x2)
        mask[:, -1:] = F.pad(torch.ones_like(_up(q, s)), (p, 0, p, 0))
        fl = [F.conv2d(F.pad(mask, pads), _w(wb, nm + ".weight").abs()) for nm, pads in
              (("conv_b1_1", (0, p, 0, p)), ("conv_b1_2", (0, p, 0, 0)), ("conv_b1_3", (0, 0, 0, p)))]
        bnd = bnd + FLOOR_DP[dp] * torch.cat(fl, 1)
    yield Layer("bd/stem", "stem", st, bnd)

    def rbs(trunk, count, seg, pool_last=False, gate=None):
        for i in range(count):
            last = i == count - 1
            name = "%s.%d" % (trunk, i)
            yield from rb_layers(get, wb, "bd", name, dp, pool=pool_last and last, gate=gate if last else None,
                                 E=(exps[seg], exps[seg + 1] if (gate is not None and last) else exps[seg]))

    def head(k, conv, src):
        h, ha = conv64(get("bd/" + src), _w(wb, conv + ".weight"), 1, _w(wb, conv + ".bias"))
        if k > 0:
            prev = get("bd/head%d" % (k - 1))[:, 0:1]
            h = torch.cat([h[:, 0:1] + prev, h[:, 1:2]], 1)
            ha = torch.cat([ha[:, 0:1] + prev.abs(), ha[:, 1:2]], 1)
        return Layer("bd/head%d" % k, "head", h, bound(ha, h, "fp32"))

    def att_input(k, S, seg):
        hk = get("bd/head%d" % k)
        a = torch.cat([_up(q, S // 8), _up(hk, S // 16)], 1)
        return Layer("bd/att_input%d" % (k + 1), "data movement", a, _store_move(a, dp, exps[seg]))

    yield from rbs("trunk_M1", 6, 0, pool_last=luma)
    yield from rbs("trunk_M2", 4, 0, pool_last=True)
    yield from rbs("trunk_B1", 3, 0)
    yield head(0, "conv_B1", "trunk_B1.2")
    yield att_input(0, 16, 1)
    yield from rbs("trunk_Att1", 2, 1, gate="trunk_M2.3")
    yield from rbs("trunk_B2", 3, 2)
    yield head(1, "conv_B2", "trunk_B2.2")
    yield att_input(1, 32, 3)
    yield from rbs("trunk_Att2", 2, 3, gate="trunk_M1.5")
    yield from rbs("trunk_B3", 3, 4, pool_last=True)
    yield head(2, "conv_B3", "trunk_B3.2")


def blocks64(luma, y, u=None, v=None):
    """The nets' input as float64: [N,1,68,68] luma, [N,3,34,34] = max_pool2d(Y) ++ U ++ V chroma (Inference_QBD.py:194-200)."""
    yt = _t(y).unsqueeze(1)
    if luma:
        return yt
    return torch.cat([F.max_pool2d(yt, 2), _t(u).unsqueeze(1), _t(v).unsqueeze(1)], 1)


def ratio(gpu, lay):
    """max |gpu - ref64| / bound over the tensor (0/0 = 0; a difference where the bound is 0 is inf)."""
    d = (gpu - lay.ref).abs()
    r = torch.where(d == 0, torch.zeros_like(d), d / lay.bound)
    return float(r.max())
