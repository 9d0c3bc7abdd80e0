"""ORACLE (test infrastructure, not product): single-tensor gains that drive one f16x3 split-2 store at a time beyond +-65504.

The range guard of the f16x3 datapath (include/pmp.h) rests on every kernel that stores a split-2 tensor raising the context's flag when
its clamp fires.  tests/test_gpu_range_sites.py checks that site by site: it over-drives ONE tensor of the graph and keeps the rest in
range, so the flag it reads can only come from that tensor's producer.

How a gain moves one tensor without changing the function.  The nets are bias-free behind their stems and heads, and ReLU, max-pool,
nearest upsampling, concat and the gate products are positively homogeneous.  Scaling a producer by s > 0 and the input channels of every
convolution that reads it by 1/s (W[:, cin_slice] only, so concatenated inputs stay right) leaves the logits as they were and multiplies
that tensor by s:
  <blk>.t            left.0 * s, left.2 / s: exactly one tensor, in every block of the four nets (also those a fused kernel keeps in LDS);
  stem / block output with a 1x1 shortcut   the producer * s (stem weights and bias; left.2 and shortcut.0), compensated at each consumer
                     (left.0 and a conv shortcut.0; the heads' weights).  A consumer block with an identity shortcut carries the gain
                     through (its left.0 / s, its left.2 * s), so the run goes on to the next conv-shortcut block; q/x6 (the multi-scale
                     pool) carries the gain of q/resblock_q3.  A gate product (gate * att, Model_QBD.py:143, :150) is compensated
                     where it is formed: a gained gate gets an attention trunk whose last block is scaled by 1/s (left.2 and its
                     conv shortcut), so the product stays and is a case of its own.  One run is one case; s is chosen from the run's
                     largest split-2 tensor (fp32_stored: the ones that cannot clamp), so that it crosses the threshold (`over`: every
                     run tensor within 3 % of it crosses too, and an fp32 one above it).
  logit-derived planes   the MTT stem's raw QT-logit plane and the attention inputs carry logits, which can be negative: the head is gained
                     with both signs of s and the convolutions that read the plane are compensated on that channel only.  The QT logits
                     feed the stem's plane and both attention inputs at once - no weight gain separates them, so that is one joint case
                     ("bd/stem.q" names the stem's plane, which has no tap).  Of the MTT heads only the direction row is gained: the depth
                     row is accumulated into the next head (Model_QBD.py:146-147, :153), the direction row reaches exactly one attention
                     input.  These cases change the logits they gain (qt, or dire[:, k], times s): their reference is the oracle on the
                     gained weights.
s_over puts the target's largest STORED value (true value / 2^E of its segment) at 1.03 x 65504, s_under at 0.97 x 65504, computed from the
float64 walk (oracle/layers64.py) on gpu_blocks(); every tensor outside the case stays below 65504 / 4 (tests/test_range_cases_cpu.py).
"""
import os

import numpy as np

from oracle import layers64 as L

LIMIT = 65504.0
OVER, UNDER = 1.03, 0.97
GOLDEN = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden")

# graph structure (Model_QBD.py) beyond what the weight names and layers64._rb_input say: the gate of each attention trunk's last block,
# the head behind each trunk, the attention input each MTT head feeds, and the multi-scale pool behind q/resblock_q3
GATES = {"trunk_Att1": "trunk_M2.3", "trunk_Att2": "trunk_M1.5"}
HEADS = {"q/resblock_q6": ("q", "conv_q2"), "bd/trunk_B1.2": ("bd", "conv_B1"), "bd/trunk_B2.2": ("bd", "conv_B2"),
         "bd/trunk_B3.2": ("bd", "conv_B3")}
ATT_HEAD = {"bd/att_input1": ("conv_B1", "trunk_Att1.0"), "bd/att_input2": ("conv_B2", "trunk_Att2.0")}
STEMS = {"q": ("conv_q1",), "bd": ("conv_b1_1", "conv_b1_2", "conv_b1_3")}
STEM_Q = "bd/stem.q"      # the MTT stem's split of the raw QT logits (conv_misc.hip): a store with no tap


def edge_blocks(n_random=2, seed=77):
    """13 luma / chroma blocks (with n_random = 2) chosen for edges: all 0, all 255, 1-pixel checkerboard, horizontal and vertical stripes,
    one bright pixel at each corner of the 68x68 block (and of the 34x34 chroma planes), two golden blocks (g1_qt.npz), recipe-R blocks."""
    from pmp_vvc_tip2023_amd import synth
    g1 = np.load(os.path.join(GOLDEN, "g1_qt.npz"), allow_pickle=False)
    ys, us, vs = [], [], []

    def add(y, u, v):
        ys.append(y.astype(np.uint8)); us.append(u.astype(np.uint8)); vs.append(v.astype(np.uint8))
    i68, i34 = np.indices((68, 68)), np.indices((34, 34))
    add(np.zeros((68, 68)), np.zeros((34, 34)), np.zeros((34, 34)))
    add(np.full((68, 68), 255), np.full((34, 34), 255), np.full((34, 34), 255))
    add(255 * ((i68[0] + i68[1]) & 1), 255 * ((i34[0] + i34[1]) & 1), 255 * ((i34[0] + i34[1] + 1) & 1))
    add(255 * (i68[0] & 1), 255 * (i34[0] & 1), 255 * (i34[1] & 1))
    add(255 * (i68[1] & 1), 255 * (i34[1] & 1), 255 * (i34[0] & 1))
    for r, c in ((0, 0), (0, -1), (-1, 0), (-1, -1)):
        y, u, v = np.zeros((68, 68)), np.zeros((34, 34)), np.zeros((34, 34))
        y[r, c] = 255; u[r, c] = 255; v[r, c] = 255
        add(y, u, v)
    for k in (0, 5):
        add(g1["block_y"][k], g1["block_u"][k], g1["block_v"][k])
    if n_random:
        ry, ru, rv = synth.recipe_r_blocks(n_random, seed)
        for k in range(n_random):
            add(ry[k], ru[k], rv[k])
    return np.stack(ys), np.stack(us), np.stack(vs)


def gpu_blocks():
    """The four blocks of the site-by-site test: all-255, the checkerboard and the two golden blocks of edge_blocks()."""
    y, u, v = edge_blocks(n_random=0)
    sel = [1, 2, 9, 10]
    return y[sel], u[sel], v[sel]


def base_weights(comp, qp=22):
    """Real QT weights and the uniform synthetic MTT weights of (comp, qp)."""
    from pmp_vvc_tip2023_amd import synth, weights as W
    wq, _ = W.load_net_weights(comp + "_Q", qp)
    return wq, synth.synth_msbd_weights(comp, qp)


def segment(name):
    """f16x3 activation-scale segment of an MTT tap (include/pmp.h; layers64.msbd_layers), None for the QT net and the logit plane."""
    if not name.startswith("bd/") or name == STEM_Q:
        return None
    n = name[3:]
    if n == "att_input1" or n.startswith("trunk_Att1.0") or n == "trunk_Att1.1.t":
        return 1
    if n == "trunk_Att1.1" or n.startswith("trunk_B2"):
        return 2
    if n == "att_input2" or n.startswith("trunk_Att2.0") or n == "trunk_Att2.1.t":
        return 3
    if n == "trunk_Att2.1" or n.startswith("trunk_B3"):
        return 4
    return 0


def walk(wq, wb, luma, x, nets=("q", "bd"), given=None):
    """The float64 walk of layers64 (fp32 constants) -> {tap or head name: float64 tensor at true scale}.  nets: which nets to walk;
    given: taps of a net that is not walked (the MTT walk reads "q/head")."""
    taps = dict(given or {})
    if "q" in nets:
        for lay in L.q_layers(taps.__getitem__, wq, luma, x, "fp32"):
            taps[lay.name] = lay.ref
    if "bd" in nets:
        for lay in L.msbd_layers(taps.__getitem__, wb, luma, x, "fp32"):
            taps[lay.name] = lay.ref
    return taps


def stored_amax(taps, name, exps=(0, 0, 0, 0, 0)):
    """Largest |stored value| of a tensor: true value / 2^E of its segment.  STEM_Q: the raw QT logits."""
    if name == STEM_Q:
        return float(taps["q/head"].abs().max())
    sg = segment(name)
    return float(taps[name].abs().max()) * 2.0 ** -(exps[sg] if sg is not None else 0)


def tap_names(taps):
    """The tap names of a walk (heads are logits, not taps)."""
    return [n for n in taps if "head" not in n]


class Case:
    """One over-drive.  name; net 'q' | 'bd' | 'qbd' (the nets whose weights change); run: the tensors that carry the gain; over: those
    pushed beyond 65504 at s_over; gains: [(net, weight name, axis, index, power)] - W.take(index, axis) *= s**power (index None: all);
    preserving: the logits stay; else out = ('qt', None) | ('dire', k): the logit tensor that is multiplied by s; sign: of s."""
    def __init__(self, name, net, run, gains, preserving=True, out=None, sign=1):
        self.name, self.net, self.run, self.gains = name, net, tuple(run), list(gains)
        self.preserving, self.out, self.sign = preserving, out, sign
        self.over = ()
        self.s_over = self.s_under = None

    def apply(self, wq, wb, s, drop=None):
        """Gained float32 copies of (wq, wb); drop: a weight name whose gain is left out (to show the checks catch a mistake)."""
        out = {"q": {k: np.array(v, np.float32, copy=True) for k, v in wq.items()},
               "bd": {k: np.array(v, np.float32, copy=True) for k, v in wb.items()}}
        for net, wname, axis, idx, power in self.gains:
            if wname == drop:
                continue
            w = out[net][wname].astype(np.float64)
            sl = [slice(None)] * w.ndim
            if idx is not None:
                sl[axis] = idx
            w[tuple(sl)] *= float(s) ** power
            out[net][wname] = w.astype(np.float32)
        return out["q"], out["bd"]

    def __repr__(self):
        return "Case(%s)" % self.name


def _blocks(w, net):
    """ResidualBlock names of a net, in launch order (weight-dict order), with their input tap."""
    names = []
    for k in w:
        if k.endswith(".left.0.weight"):
            names.append(k[:-len(".left.0.weight")])
    return [(b, net + "/" + L._rb_input(net, b)) for b in names]


def _gated(block):
    """The gate of a block's output (the last block of an attention trunk), or None."""
    trunk, i = block.rsplit(".", 1) if "." in block else (block, "")
    return GATES.get(trunk) if i == "1" else None


def build_cases(wq, wb):
    """Every case of one component's (QT, MTT) pair, generated from the weight names and the graph tables above; s is not set yet."""
    nets = {"q": wq, "bd": wb}
    blocks = {net: _blocks(w, net) for net, w in nets.items()}
    cases = []
    # .t: one tensor per block
    for net, bl in blocks.items():
        for b, _ in bl:
            cases.append(Case("%s/%s.t" % (net, b), net, ["%s/%s.t" % (net, b)],
                              [(net, b + ".left.0.weight", 0, None, 1), (net, b + ".left.2.weight", 0, None, -1)]))

    # runs: from each stem and each block output with a conv shortcut, through identity blocks, x6 and gate products
    def consumers(node):
        net = node.split("/")[0]
        for b, inp in blocks[net]:
            if inp == node:
                yield ("block", net, b)
        if node == "q/resblock_q3":
            yield ("move", "q", "q/x6")
        for b, _ in blocks.get("bd", []):
            g = _gated(b)
            if g is not None and node == "bd/" + g:
                yield ("gate", "bd", "bd/" + b)
        if node in HEADS:
            yield ("head",) + HEADS[node]

    starts = [(net + "/stem", [(net, c + sfx, 0, None, 1) for c in STEMS[net] for sfx in (".weight", ".bias")]) for net in nets]
    for net, bl in blocks.items():
        for b, _ in bl:
            if b + ".shortcut.0.weight" in nets[net]:
                starts.append(("%s/%s" % (net, b), [(net, b + ".left.2.weight", 0, None, 1), (net, b + ".shortcut.0.weight", 0, None, 1)]))
    for node0, gains in starts:
        run, todo, gains = [node0], [node0], list(gains)
        while todo:
            node = todo.pop(0)
            for kind, net, what in consumers(node):
                if kind == "block":
                    gains.append((net, what + ".left.0.weight", 1, None, -1))
                    if what + ".shortcut.0.weight" in nets[net]:
                        gains.append((net, what + ".shortcut.0.weight", 1, None, -1))
                        nxt = None
                    else:
                        gains.append((net, what + ".left.2.weight", 0, None, 1))
                        nxt = "%s/%s" % (net, what)
                elif kind == "head":
                    gains.append((net, what + ".weight", 1, None, -1))
                    nxt = None
                elif kind == "gate":        # gate * att: the attention trunk's last block (a conv shortcut) takes the 1/s
                    blk = what.split("/")[1]
                    gains += [(net, blk + ".left.2.weight", 0, None, -1), (net, blk + ".shortcut.0.weight", 0, None, -1)]
                    nxt = None
                else:                       # x6: the gain passes through
                    nxt = what
                if nxt is not None and nxt not in run:
                    run.append(nxt)
                    todo.append(nxt)
        cases.append(Case(node0 if len(run) == 1 else "%s..%s" % (node0, run[-1].split("/")[1]), node0.split("/")[0], run, gains))

    # logit-derived planes, both signs
    qcomp = [("bd", c + ".weight", 1, -1, -1) for c in STEMS["bd"]]
    for att, (_, blk) in ATT_HEAD.items():
        qcomp += [("bd", blk + ".left.0.weight", 1, 0, -1), ("bd", blk + ".shortcut.0.weight", 1, 0, -1)]
    for sign in (1, -1):
        sg = "+" if sign > 0 else "-"
        cases.append(Case("q/head%s" % sg, "qbd", [STEM_Q] + sorted(ATT_HEAD),
                          [("q", "conv_q2.weight", 0, None, 1), ("q", "conv_q2.bias", 0, None, 1)] + qcomp,
                          preserving=False, out=("qt", None), sign=sign))
        for k, (att, (head, blk)) in enumerate(sorted(ATT_HEAD.items())):
            cases.append(Case("bd/head%d.dire%s" % (k, sg), "bd", [att],
                              [("bd", head + ".weight", 0, 1, 1), ("bd", head + ".bias", 0, 1, 1),
                               ("bd", blk + ".left.0.weight", 1, 2, -1), ("bd", blk + ".shortcut.0.weight", 1, 2, -1)],
                              preserving=False, out=("dire", k), sign=sign))
    return cases


def _gained_amax(case, base, name, exps):
    """Largest stored value of the part of a run tensor that carries the gain, per unit of s (from the ungained walk)."""
    if case.preserving:
        return stored_amax(base, name, exps)
    if case.out[0] == "qt":                      # the logit channel of the plane
        q = float(base["q/head"].abs().max())
        return q * 2.0 ** -(exps[segment(name)] if segment(name) is not None else 0)
    k = case.out[1]
    return float(base["bd/head%d" % k][:, 1].abs().max()) * 2.0 ** -exps[segment(name)]


def fp32_stored(name, base):
    """True where the graph stores a tensor in plain fp32 (never clamped, no flag) because its consumer is no MFMA convolution
    (csrc/nets.cpp): the multi-scale pool reads q/resblock_q3, a head reads the last block of a trunk, and the 8x8 layers run the direct
    fp32 kernel - their input, intermediate and output (layers64: `direct`, a block input of at most 8x8)."""
    if name == STEM_Q:
        return False
    return name == "q/resblock_q3" or name in HEADS or base[name].shape[-1] <= 8


def set_gains(case, base, exps=(0, 0, 0, 0, 0)):
    """s_over, s_under and the tensors that cross at s_over, from the ungained walk `base` (linear in s: every gained part is s x base).
    s comes from the run's largest SPLIT-2 tensor - the stores that can clamp - so that a run whose largest tensor is stored in fp32
    (q/resblock_q4..resblock_q5) still over-drives its split-2 one; the fp32 ones then sit unclamped above 65504."""
    amax = {n: _gained_amax(case, base, n, exps) for n in case.run}
    split = [a for n, a in amax.items() if not fp32_stored(n, base)]
    top = max(split or amax.values())
    case.s_over = case.sign * OVER * LIMIT / top
    case.s_under = case.sign * UNDER * LIMIT / top
    case.over = tuple(n for n in case.run if amax[n] * abs(case.s_over) > LIMIT)
    return case


def cases_for(comp, x=None):
    """(cases with their gains set, ungained walk, (wq, wb), x float64 input) of a component on gpu_blocks()."""
    luma = comp == "Luma"
    wq, wb = base_weights(comp)
    if x is None:
        y, u, v = gpu_blocks()
        x = L.blocks64(luma, y, u, v)
    base = walk(wq, wb, luma, x)
    return [set_gains(c, base) for c in build_cases(wq, wb)], base, (wq, wb), x


# one case per MTT segment with non-zero exponents (f16x3 activation scales from a .pmpw manifest): the tensor each over-drives
SEGMENT_EXPS = (3, 2, 4, 3, 5)
SEGMENT_TARGETS = ("bd/trunk_B1.0", "bd/trunk_Att1.0.t", "bd/trunk_Att1.1", "bd/trunk_Att2.0.t", "bd/trunk_B3.1")


def segment_cases(cases, base, exps=SEGMENT_EXPS):
    """Copies of the single-tensor cases named in SEGMENT_TARGETS, gains set in stored units (true x 2^-E) under `exps`."""
    out = []
    for tgt in SEGMENT_TARGETS:
        c = next(c for c in cases if c.run == (tgt,))
        sc = Case("E%s:%s" % ("".join(map(str, exps)), c.name), c.net, c.run, c.gains)
        out.append(set_gains(sc, base, exps))
    return out


def logit_gain(case, s):
    """What the case does to the logits (qt, bt, dire): a multiplier per output, s on the gained one, 1 elsewhere."""
    g = {"qt": 1.0, "bt": np.ones(3), "dire": np.ones(3)}
    if not case.preserving:
        if case.out[0] == "qt":
            g["qt"] = abs(s)
        else:
            g["dire"][case.out[1]] = abs(s)
    return g


def logit_err(got, ref, case, s):
    """max |got - ref| over (qt, bt, dire), each divided by |s| where the case multiplies that logit by s."""
    g = logit_gain(case, s)
    e = float(np.abs(got[0] - ref[0]).max()) / g["qt"]
    for k in range(3):
        e = max(e, float(np.abs(got[1][:, k] - ref[1][:, k]).max()) / g["bt"][k],
                float(np.abs(got[2][:, k] - ref[2][:, k]).max()) / g["dire"][k])
    return e

