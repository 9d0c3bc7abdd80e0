"""GPU: a trunk of ResidualBlocks kept blocked, with pool, forward and backward (include/pmp.h: pmp_trunk_*; csrc/api_train.cpp,
trunk_glue.hip; pmp_vvc_tip2023_amd/trunk.py).

Bounds.  On the EXACT cases of tests/trunk_cases.py every value is an integer below 2^24, float32 arithmetic is exact in any order, and
every result - y, every saved t_i and out_i, g_x, every weight gradient - must equal the float64 restatement BIT FOR BIT, no element
left out, in poisoned workspaces, into NaN-filled outputs and a NaN-filled d_saved.  On float values the trunk must equal the chain of
pmp_resblock_*_device calls through dense tensors with torch's max_pool2d, again bit for bit: both sides run the same convolution
and weight-gradient kernels on the same values in the same order, and everything in between is a copy, a select or a maximum."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import resblock_cases as K
import trunk_cases as T

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    from pmp_vvc_tip2023_amd import engine
    assert torch.cuda.is_available()
    torch.set_num_threads(16)
    e = engine.Engine(0)
    yield e
    e._ck(e.lib.pmp_debug_poison_workspace(e.h, 0))
    e.close()


@functools.lru_cache(maxsize=None)
def exact(name):
    """-> (case, the float64 restatement as the float32 a kernel must produce, flat); computed once, never changed."""
    c = T.make_exact(name)
    return c, {k: K.as_f32(v) for k, v in T.flat(T.restate(c)).items()}


def P(t):
    return None if t is None else t.data_ptr()


def up(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda()


def nan(*shape):
    return torch.full(shape, float("nan"), device="cuda")


class Dev:
    """A case on the device: inputs, NaN-filled outputs and a NaN-filled saved buffer (0xFF bytes)."""

    def __init__(self, e, c, pool=None):
        n, h, w, cin, blocks, p = c["shape"]
        self.shape = (n, h, w, cin, blocks, p if pool is None else pool)
        self.x, self.g_y = up(c["x"]), up(c["g_y"])
        self.w = [up(a) for blk in c["blocks"] for a in blk]
        self.saved = torch.full((e.trunk_saved_bytes(self.shape),), 0xFF, dtype=torch.uint8, device="cuda")
        self.y = nan(*T.y_shape(self.shape))
        self.g_x = nan(n, cin, h, w)
        self.g_w = [None if a is None else nan(*a.shape) for a in self.w]
        torch.cuda.synchronize()

    def forward(self, e):
        e.trunk_forward_device(self.shape, P(self.x), [P(a) for a in self.w], P(self.saved), P(self.y))

    def backward(self, e, want_g_x=True):
        e.trunk_backward_device(self.shape, P(self.saved), [P(a) for a in self.w], P(self.g_y), P(self.g_x) if want_g_x else None,
                                [P(a) for a in self.g_w])

    def unpack(self, e):
        """-> (t, out): lists of dense device tensors, through pmp_trunk_unpack_device into NaN-filled buffers."""
        n, h, w = self.shape[:3]
        ts, outs = [], []
        for i, (cout, _) in enumerate(self.shape[4]):
            ts.append(nan(n, cout, h, w))
            outs.append(nan(n, cout, h, w))
            torch.cuda.synchronize()                 # torch fills them on ITS stream: done before the engine's stream writes them
            e.trunk_unpack_device(self.shape, P(self.saved), 2 * i + 1, P(ts[-1]))
            e.trunk_unpack_device(self.shape, P(self.saved), 2 * i + 2, P(outs[-1]))
        return ts, outs

    def results(self, e, ts=None, outs=None):
        """Everything the calls produced, flat like trunk_cases.flat (g_x the untouched NaN buffer if it was not asked for)."""
        if ts is None:
            ts, outs = self.unpack(e)
        x0 = nan(*self.x.shape)
        torch.cuda.synchronize()
        e.trunk_unpack_device(self.shape, P(self.saved), 0, P(x0))
        e.synchronize()
        num = lambda a: None if a is None else a.cpu().numpy()
        r = T.flat({"y": num(self.y), "g_x": num(self.g_x), "t": [num(a) for a in ts], "out": [num(a) for a in outs],
                    "g_w": [tuple(num(a) for a in self.g_w[3 * i:3 * i + 3]) for i in range(len(ts))]})
        r["x"] = num(x0)
        return r


def run(e, c, want_g_x=True, pool=None):
    d = Dev(e, c, pool)
    d.forward(e)
    d.backward(e, want_g_x)
    return d.results(e)


def check_bits(what, got, want, skip=()):
    for k, v in want.items():
        if k in skip:
            continue
        assert got[k].dtype == np.float32 and K.same_bits(got[k], v), (what, k, np.argwhere(~(got[k] == v))[:4])


# ---- 1. every exact case equals the restatement, in poisoned workspaces, into NaN-filled outputs and a NaN-filled d_saved
@pytest.mark.parametrize("name", list(T.EXACT))
def test_exact_cases_bit_equal(eng, name):
    c, want = exact(name)
    for pattern in (1, 2):
        eng._ck(eng.lib.pmp_debug_poison_workspace(eng.h, pattern))
        got = run(eng, c)
        assert sorted(k for k in got if k != "x") == sorted(want)
        check_bits("poison %d" % pattern, got, want)
        assert K.same_bits(got["x"], c["x"]), "unpack of x"
    eng._ck(eng.lib.pmp_debug_poison_workspace(eng.h, 0))


# ---- 2. float values: the trunk is the chain of pmp_resblock_*_device calls through dense tensors, plus torch's max_pool2d
def chain(e, c, ts_in, outs_in):
    """The parent's API: forward block by block, y by torch; backward block by block on the GIVEN t_i and out_i -> flat results."""
    n, h, w = c["shape"][:3]
    pool = c["shape"][5]
    x = up(c["x"])
    ws = [tuple(up(a) for a in blk) for blk in c["blocks"]]
    ts, outs, xs = [], [], [x]
    for (ci, co, k), (w0, w2, wsc) in zip(T.block_shapes(c["shape"]), ws):
        t, out = nan(n, co, h, w), nan(n, co, h, w)
        torch.cuda.synchronize()                     # (as in Dev.unpack: the NaN fills must not overtake the engine's kernels)
        e.resblock_forward_device((n, h, w, ci, co, k), P(xs[-1]), P(w0), P(w2), P(wsc), P(t), P(out))
        ts.append(t); outs.append(out); xs.append(out)
    e.synchronize()
    y = F.max_pool2d(outs[-1], 2) if pool else outs[-1]
    g = up(c["g_y"])
    if pool:
        o = outs_in[-1].detach().clone().requires_grad_()
        g, = torch.autograd.grad(F.max_pool2d(o, 2), o, g)
        g = g.contiguous()
    torch.cuda.synchronize()
    g_w = [None] * len(ws)
    for i in range(len(ws) - 1, -1, -1):
        ci, co, k = T.block_shapes(c["shape"])[i]
        w0, w2, wsc = ws[i]
        x_i = x if i == 0 else outs_in[i - 1]
        g_x, gw = nan(n, ci, h, w), tuple(None if a is None else nan(*a.shape) for a in ws[i])
        torch.cuda.synchronize()
        e.resblock_backward_device((n, h, w, ci, co, k), P(x_i), P(ts_in[i]), P(outs_in[i]), P(w0), P(w2), P(wsc), P(g), P(g_x), P(gw[0]), P(gw[1]),
                                   P(gw[2]))
        g_w[i], g = gw, g_x
    e.synchronize()
    num = lambda a: None if a is None else a.cpu().numpy()
    return T.flat({"y": num(y), "g_x": num(g), "t": [num(a) for a in ts], "out": [num(a) for a in outs],
                   "g_w": [tuple(num(a) for a in gw) for gw in g_w]})


@pytest.mark.parametrize("name", ["f_m1_like", "f_b3_like"])
def test_trunk_equals_chain_of_block_calls(eng, name):
    c = T.make_float(name)
    d = Dev(eng, c)
    d.forward(eng)
    d.backward(eng)
    ts, outs = d.unpack(eng)
    eng.synchronize()
    got = d.results(eng, ts, outs)
    want = chain(eng, c, ts, outs)
    assert sorted(k for k in got if k != "x") == sorted(want)
    for k, v in want.items():
        assert np.isfinite(v).all() and np.abs(v).max() > 0, (name, k)
    check_bits(name, got, want)


# ---- 3. optional and variant paths
@pytest.mark.parametrize("name", ["one_pool", "att_like"])
def test_without_g_x(eng, name):
    c, want = exact(name)
    got = run(eng, c, want_g_x=False)
    assert np.isnan(got["g_x"]).all()
    check_bits("no g_x", got, want, skip=("g_x",))


def test_pool_and_no_pool_agree_on_the_saved_tensors(eng):
    c = T.make_float("f_b3_like")
    a, b = Dev(eng, c, pool=1), Dev(eng, c, pool=0)
    a.forward(eng)
    b.forward(eng)
    ra, rb = a.results(eng), b.results(eng)
    for k in ra:
        if k == "x" or k.startswith("t") or k.startswith("out"):
            assert not np.isnan(ra[k]).any() and K.same_bits(ra[k], rb[k]), k
    last = "out%d" % (len(c["blocks"]) - 1)
    assert K.same_bits(rb["y"], rb[last]) and K.same_bits(ra["y"], T.pool(ra[last]))
    assert torch.equal(a.saved, b.saved)                 # the whole opaque buffer, padded channels included


# ---- 4. determinism: twice, on a second stream, on a second context
def test_same_bits_on_every_run_stream_and_context(eng):
    from pmp_vvc_tip2023_amd import engine
    c = T.make_float("f_m1_like")
    first = run(eng, c)
    runs = {"again": run(eng, c)}
    side = torch.cuda.Stream()
    eng.set_stream(side.cuda_stream)
    try:
        runs["second stream"] = run(eng, c)
    finally:
        eng.set_stream(0)
    e2 = engine.Engine(0)
    try:
        side2 = torch.cuda.Stream()
        e2.set_stream(side2.cuda_stream)
        runs["second context on another stream"] = run(e2, c)
    finally:
        e2.close()
    for what, r in runs.items():
        for k, v in first.items():
            assert not np.isnan(v).any() and K.same_bits(r[k], v), (what, k)


# ---- 5. refusals: PMP_E_INVALID before any launch, nothing written
def test_refusals_write_nothing(eng):
    from pmp_vvc_tip2023_amd import _lib
    cs = {nm: exact(nm)[0] for nm in ("one_pool", "b_like")}           # identity shortcuts only / conv shortcuts only
    dev = {nm: Dev(eng, c) for nm, c in cs.items()}
    ok = Dev(eng, cs["one_pool"])                                      # a finished forward, for the calls that read d_saved
    ok.forward(eng)
    eng.synchronize()
    saved_ok = ok.saved.clone()
    dense = nan(*ok.x.shape)
    other = up(cs["b_like"]["blocks"][0][2])                           # some shortcut tensor
    other_g = nan(*other.shape)
    arr = lambda ps: (C.c_void_p * len(ps))(*ps)

    def call(nm, what, shape=None, null_shape=False, w=None, g_w=None, null_w=False, null_g_w=False, index=1, **swap):
        d = ok if what != "forward" and nm == "one_pool" else dev[nm]
        p = {"x": P(d.x), "saved": P(d.saved), "y": P(d.y), "g_y": P(d.g_y), "g_x": P(d.g_x), "dense": P(dense)}
        p.update(swap)
        ws, gws = [P(a) for a in d.w], [P(a) for a in d.g_w]
        for i, v in (w or {}).items():
            ws[i] = v
        for i, v in (g_w or {}).items():
            gws[i] = v
        s = _lib.trunk_shape(shape or d.shape)
        sp = None if null_shape else C.byref(s)
        wa, ga = None if null_w else arr(ws), None if null_g_w else arr(gws)
        if what == "forward":
            return eng.lib.pmp_trunk_forward_device(eng.h, sp, p["x"], wa, p["saved"], p["y"])
        if what == "backward":
            return eng.lib.pmp_trunk_backward_device(eng.h, sp, p["saved"], wa, p["g_y"], p["g_x"], ga)
        return eng.lib.pmp_trunk_unpack_device(eng.h, sp, p["saved"], index, p["dense"])

    n, h, w, cin, blocks, pool = cs["one_pool"]["shape"]
    bad_shapes = [(0, h, w, cin, blocks, pool), (257, h, w, cin, blocks, pool), (n, 8, w, cin, blocks, pool), (n, 24, w, cin, blocks, pool),
                  (n, 272, w, cin, blocks, pool), (n, h, 0, cin, blocks, pool), (n, h, 40, cin, blocks, pool), (n, h, w, 0, blocks, pool),
                  (n, h, w, 65, blocks, pool), (n, h, w, cin, [], pool), (n, h, w, cin, [(16, 3)] * 9, pool), (n, h, w, cin, [(0, 3)], pool),
                  (n, h, w, cin, [(65, 3)], pool), (n, h, w, cin, [(16, 1)], pool), (n, h, w, cin, [(16, 4)], pool), (n, h, w, cin, [(16, 7)], pool),
                  (n, h, w, cin, blocks, 2), (n, h, w, cin, blocks, -1)]
    tries = []
    for what in ("forward", "backward", "unpack"):
        tries += [("shape %s" % (s,), "one_pool", what, dict(shape=s)) for s in bad_shapes]
        tries += [("null shape", "one_pool", what, dict(null_shape=True)), ("null d_saved", "one_pool", what, dict(saved=None)),
                  ("misaligned d_saved (8 bytes)", "one_pool", what, dict(saved=P(ok.saved) + 8))]
    for what in ("forward", "backward"):
        tries += [("null d_w", "one_pool", what, dict(null_w=True)), ("null w0", "one_pool", what, dict(w={0: None})),
                  ("null w2", "b_like", what, dict(w={4: None})),
                  ("wsc with an identity shortcut", "one_pool", what, dict(w={2: P(other)}, g_w={2: P(other_g)})),
                  ("no wsc with a conv shortcut", "b_like", what, dict(w={5: None}, g_w={5: None})),
                  # cin != cout in block 0 of a shape whose tensors are an identity block's
                  ("a shape with a shortcut, tensors without", "one_pool", what, dict(shape=(n, h, w, cin, [(8, 3)], pool))),
                  ("misaligned w0", "one_pool", what, dict(w={0: P(dev["one_pool"].w[0]) + 2}))]
    o = dev["one_pool"]
    tries += [("null x", "one_pool", "forward", dict(x=None)), ("null y", "one_pool", "forward", dict(y=None)),
              ("y overlaps x", "one_pool", "forward", dict(y=P(o.x) + 64)), ("y inside d_saved", "one_pool", "forward", dict(y=P(o.saved) + 256)),
              ("d_saved overlaps w2", "one_pool", "forward", dict(saved=P(o.w[1]))), ("d_saved is x", "one_pool", "forward", dict(saved=P(o.x))),
              ("misaligned x", "one_pool", "forward", dict(x=P(o.x) + 2)), ("misaligned y", "one_pool", "forward", dict(y=P(o.y) + 1)),
              ("null g_y", "one_pool", "backward", dict(g_y=None)), ("null d_g_w", "one_pool", "backward", dict(null_g_w=True)),
              ("null g_w0", "one_pool", "backward", dict(g_w={0: None})), ("null g_w2", "b_like", "backward", dict(g_w={7: None})),
              ("g_wsc with an identity shortcut", "one_pool", "backward", dict(g_w={2: P(other_g)})),
              ("no g_wsc with a conv shortcut", "b_like", "backward", dict(g_w={2: None})),
              ("g_x overlaps g_y", "one_pool", "backward", dict(g_x=P(ok.g_y))), ("g_x inside d_saved", "one_pool", "backward", dict(g_x=P(ok.saved) + 1024)),
              ("g_w0 is g_w2", "one_pool", "backward", dict(g_w={0: P(ok.g_w[1])})), ("g_w2 overlaps w0", "one_pool", "backward", dict(g_w={1: P(ok.w[0]) + 4})),
              ("g_w0 overlaps g_x", "one_pool", "backward", dict(g_w={0: P(ok.g_x) + 16})),
              ("misaligned g_w0", "one_pool", "backward", dict(g_w={0: P(ok.g_w[0]) + 2})), ("misaligned g_y", "one_pool", "backward", dict(g_y=P(ok.g_y) + 2)),
              ("null dense", "one_pool", "unpack", dict(dense=None)), ("index -1", "one_pool", "unpack", dict(index=-1)),
              ("index 3 of one block", "one_pool", "unpack", dict(index=3)), ("dense inside d_saved", "one_pool", "unpack", dict(dense=P(ok.saved) + 512)),
              ("misaligned dense", "one_pool", "unpack", dict(dense=P(dense) + 2))]
    for what, nm, which, kw in tries:
        assert call(nm, which, **kw) == -1, (what, which)
        assert eng.lib.pmp_last_error(eng.h), what
    eng.synchronize()
    torch.cuda.synchronize()
    for nm, d in list(dev.items()) + [("ok", ok)]:
        for k, a in [("y", d.y), ("g_x", d.g_x)] + [("g_w%d" % i, a) for i, a in enumerate(d.g_w) if a is not None]:
            assert nm == "ok" and k == "y" or torch.isnan(a).all(), (nm, k, "written by a refused call")
        if nm != "ok":
            assert (d.saved == 0xFF).all(), (nm, "d_saved written by a refused call")
        c = cs["one_pool" if nm == "ok" else nm]
        assert K.same_bits(d.x.cpu().numpy(), c["x"]) and K.same_bits(d.g_y.cpu().numpy(), c["g_y"])
        for a, src in zip(d.w, [a for blk in c["blocks"] for a in blk]):
            assert a is None or K.same_bits(a.cpu().numpy(), src), nm
    assert torch.isnan(dense).all() and torch.isnan(other_g).all() and torch.equal(ok.saved, saved_ok)
    # and the calls after a refusal still work
    ok.backward(eng)
    check_bits("after the refusals", ok.results(eng), exact("one_pool")[1])


# ---- 6. under torch.autograd, on CUDA tensors: the trunk function against the chain of block functions and F.max_pool2d
@pytest.mark.parametrize("side_stream", [False, True])
def test_autograd_function_equals_chain_of_block_functions(eng, side_stream):
    from pmp_vvc_tip2023_amd import resblock, trunk
    c = T.make_float("f_m2_like")

    def leaves():
        return up(c["x"]).requires_grad_(), [tuple(None if a is None else up(a).requires_grad_() for a in blk) for blk in c["blocks"]]

    def grads(x, ws):
        torch.cuda.synchronize()
        return [x.grad.cpu().numpy()] + [a.grad.cpu().numpy() for blk in ws for a in blk if a is not None]

    try:
        with torch.cuda.stream(torch.cuda.Stream() if side_stream else torch.cuda.default_stream()):
            g_y = up(c["g_y"])
            x, ws = leaves()
            y = trunk.trunk(eng, x, ws, pool=True)
            y.backward(g_y)
            got = [y.detach().cpu().numpy()] + grads(x, ws)
            x, ws = leaves()
            a = x
            for w0, w2, wsc in ws:
                a = resblock.residual_block(eng, a, w0, w2, wsc)
            y = F.max_pool2d(a, 2)
            y.backward(g_y)
            want = [y.detach().cpu().numpy()] + grads(x, ws)
            # x without a gradient: none comes back, and the weights' are the same
            x, ws = leaves()
            trunk.trunk(eng, x.detach(), ws, pool=True).backward(g_y)
            torch.cuda.synchronize()
            assert x.grad is None
            no_gx = [a.grad.cpu().numpy() for blk in ws for a in blk if a is not None]
    finally:
        eng.set_stream(0)
    assert len(got) == len(want) == 2 + 2 * len(c["blocks"])
    for i, (a, b) in enumerate(zip(got, want)):
        assert np.isfinite(b).all() and np.abs(b).max() > 0 and K.same_bits(a, b), i
    for i, (a, b) in enumerate(zip(no_gx, want[2:])):
        assert K.same_bits(a, b), i


class _Block(torch.nn.Module):
    """The attributes trunk_of reads of a Model_QBD.ResidualBlock."""

    def __init__(self, w0, w2, wsc):
        super().__init__()
        par = lambda a: torch.nn.Parameter(torch.from_numpy(a))
        conv = lambda a: torch.nn.Conv2d(a.shape[1], a.shape[0], a.shape[2], padding=a.shape[2] // 2, bias=False)
        self.left = torch.nn.Sequential(conv(w0), torch.nn.ReLU(inplace=True), conv(w2))
        self.left[0].weight, self.left[2].weight = par(w0), par(w2)
        self.shortcut = torch.nn.Sequential()
        if wsc is not None:
            wsc4 = wsc.reshape(wsc.shape[0], wsc.shape[1], 1, 1)
            self.shortcut = torch.nn.Sequential(conv(wsc4))
            self.shortcut[0].weight = par(wsc4)


def test_trunk_of_a_sequential(eng):
    c, want = exact("b3_like")
    seq = torch.nn.Sequential(*[_Block(*blk) for blk in c["blocks"]]).cuda()
    from pmp_vvc_tip2023_amd import trunk
    try:
        x = up(c["x"]).requires_grad_()
        y = trunk.trunk_of(eng, seq, x, pool=True)
        y.backward(up(c["g_y"]))
        torch.cuda.synchronize()
    finally:
        eng.set_stream(0)
    got = {"y": y.detach().cpu().numpy(), "g_x": x.grad.cpu().numpy()}
    for i, m in enumerate(seq):
        got["g_w0_%d" % i], got["g_w2_%d" % i] = m.left[0].weight.grad.cpu().numpy(), m.left[2].weight.grad.cpu().numpy()
        if len(m.shortcut):
            got["g_wsc_%d" % i] = m.shortcut[0].weight.grad.cpu().numpy().reshape(want["g_wsc_%d" % i].shape)
    check_bits("trunk_of", got, {k: v for k, v in want.items() if k in got})
    assert sorted(got) == sorted(T.golden_keys(want))
