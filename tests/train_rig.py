"""The rig of the training calls' GPU tests (test_gpu_resblock_grad, test_gpu_trunk_grad, test_gpu_qtail_grad, test_gpu_stem_grad,
test_gpu_head_grad, the two sweeps and test_gpu_api_sequences_train): the engine fixture, tensors to and from the device, the bit check,
a case of each call on the device (BlockDev, ChainDev as TrunkDev and TailDev, StemDev, HeadDev: the only parts that name a call's
tensors), the determinism check and the harness of the refusal tests.  A plain module: every test file
keeps its own cases, bounds and tables."""
import ctypes as C

import numpy as np
import torch
import torch.nn.functional as F

import gpu_rig
import head_cases as H
import stem_cases as S
import trunk_cases as T
from cases_common import same_bits


def engine_fixture(poison=0):
    """-> a module-scoped fixture: an Engine of the module's own, its workspaces poisoned with pattern `poison` from the start."""
    return gpu_rig.engine_fixture(poison=poison, threads=16)


def P(t):
    return None if t is None else t.data_ptr()


def up(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda()


def nan(*shape):
    return torch.full(shape, float("nan"), device="cuda")


def num(a):
    return None if a is None else a.cpu().numpy()


def torch_done():
    """Call between filling a buffer through torch and handing it to the engine.  torch fills and copies on ITS stream, the engine's
    kernels run on the engine's, and nothing orders the two: without this a NaN fill still queued on torch's stream can be overtaken
    by the engine's kernels and land on top of their results (or an upload arrive after the kernel that reads it)."""
    torch.cuda.synchronize()


def check_bits(what, got, want, keys=None, skip=()):
    """got[k] is float32 and equals want[k] bit for bit, for every k of keys (default: all of want) not in skip; a None in want
    means absent in got."""
    for k in want if keys is None else keys:
        if k in skip:
            continue
        if want[k] is None:
            assert k not in got or got[k] is None, (what, k)
            continue
        assert got[k].dtype == np.float32 and same_bits(got[k], want[k]), (what, k, np.argwhere(~(got[k] == want[k]))[:4])


def check_bits_same_keys(what, got, want, skip=()):
    """check_bits, and got holds exactly the keys of want (the stem's tests)."""
    assert sorted(got) == sorted(want)
    check_bits(what, got, want, skip=skip)


class Off4:
    """A device tensor whose first element lies 4 bytes behind a 16-byte boundary, inside a NaN-filled buffer."""

    def __init__(self, t):
        n = t.numel()
        self.buf = torch.full((n + 8,), float("nan"), device="cuda")
        self.view = self.buf[1:1 + n].view(t.shape)
        self.view.copy_(t)
        assert self.buf.data_ptr() % 16 == 0 and self.view.data_ptr() % 16 == 4 and self.view.is_contiguous()

    def guards_intact(self):
        return bool(torch.isnan(self.buf[0])) and bool(torch.isnan(self.buf[1 + self.view.numel():]).all())


def reference_block(w0, w2, wsc):
    """The attributes residual_block_of and trunk_of read of a Model_QBD.ResidualBlock, with the given weights (numpy; wsc [cout,
    cin] or None)."""
    par = lambda a: torch.nn.Parameter(torch.from_numpy(a))
    conv = lambda a: torch.nn.Conv2d(a.shape[1], a.shape[0], a.shape[2], padding=a.shape[2] // 2, bias=False)
    m = torch.nn.Module()
    m.left = torch.nn.Sequential(conv(w0), torch.nn.ReLU(inplace=True), conv(w2))
    m.left[0].weight, m.left[2].weight = par(w0), par(w2)
    m.shortcut = torch.nn.Sequential()
    if wsc is not None:
        wsc4 = wsc.reshape(wsc.shape[0], wsc.shape[1], 1, 1)
        m.shortcut = torch.nn.Sequential(conv(wsc4))
        m.shortcut[0].weight = par(wsc4)
    return m


# ---- one ResidualBlock: pmp_resblock_forward_device / pmp_resblock_backward_device
FWD_IN, BWD_IN = ("x", "w0", "w2", "wsc"), ("x", "t", "out", "w0", "w2", "wsc", "g_out")
GRADS = ("g_x", "g_w0", "g_w2", "g_wsc")


def shape_of(c, key):
    n, h, w, cin, cout, k = c["shape"]
    return {"x": (n, cin, h, w), "g_x": (n, cin, h, w), "t": (n, cout, h, w), "out": (n, cout, h, w), "g_out": (n, cout, h, w),
            "w0": (cout, cin, k, k), "g_w0": (cout, cin, k, k), "w2": (cout, cout, k, k), "g_w2": (cout, cout, k, k),
            "wsc": (cout, cin), "g_wsc": (cout, cin)}[key]


def nan_dev(c, keys):
    return {k: nan(*shape_of(c, k)) for k in keys}


class BlockDev:
    """A block case on the device: the inputs `ins` of it as .d, NaN-filled outputs `outs` as .o (g_wsc only with a shortcut)."""

    def __init__(self, c, ins=BWD_IN, outs=("t", "out") + GRADS):
        self.shape = c["shape"]
        self.d = {k: up(c[k]) for k in ins}
        self.o = nan_dev(c, [k for k in outs if c["wsc"] is not None or k != "g_wsc"])
        torch_done()

    def forward(self, e):
        e.resblock_forward_device(self.shape, *[P(self.d[k]) for k in FWD_IN], P(self.o["t"]), P(self.o["out"]))

    def backward(self, e, want_g_x=True):
        o = self.o
        e.resblock_backward_device(self.shape, *[P(self.d[k]) for k in BWD_IN], P(o["g_x"]) if want_g_x else None, P(o["g_w0"]), P(o["g_w2"]),
                                   P(o.get("g_wsc")))

    def results(self, e):
        e.synchronize()
        return {k: num(v) for k, v in self.o.items()}


def dev_forward(e, c):
    d = BlockDev(c, FWD_IN, ("t", "out"))
    d.forward(e)
    return d.results(e)


def dev_backward(e, c, want_g_x=True):
    """-> the gradients from the case's own t and out; g_x comes back as the untouched NaN buffer when it is not asked for (it is
    not passed)."""
    d = BlockDev(c, BWD_IN, GRADS)
    d.backward(e, want_g_x)
    return d.results(e)


def run_block(e, c):
    return dict(dev_forward(e, c), **dev_backward(e, c))


def _np(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def host_calls(e, c):
    """The host forms through the library itself, into NaN-filled numpy buffers -> (rc forward, rc backward, outputs)."""
    from pmp_vvc_tip2023_amd import _lib
    s = _lib.RbShape(*c["shape"])
    a = {k: None if c[k] is None else np.ascontiguousarray(c[k], np.float32) for k in BWD_IN}
    sc = c["wsc"] is not None
    o = {k: np.full(shape_of(c, k), np.nan, np.float32) for k in ("t", "out") + GRADS if sc or k != "g_wsc"}
    rf = e.lib.pmp_resblock_forward(e.h, C.byref(s), *[_np(a[k]) for k in FWD_IN], _np(o["t"]), _np(o["out"]))
    rb = e.lib.pmp_resblock_backward(e.h, C.byref(s), *[_np(a[k]) for k in BWD_IN], *[_np(o.get(k)) for k in GRADS])
    return rf, rb, o


# ---- a chain with a saved buffer: pmp_trunk_* and pmp_qtail_* (forward_device / backward_device / unpack_device)
class ChainDev:
    """A case of a chain on the device: inputs, NaN-filled outputs and a saved buffer of 0xFF bytes (NaNs, read as floats).  The two
    variants say which calls (CALLS), how the case names x, y, g_y and g_x (NAMES), the shapes and unpack's indices."""

    def __init__(self, e, c, shape, y_shape):
        self.shape = shape
        self.x, self.g_y = up(c[self.NAMES[0]]), up(c[self.NAMES[2]])
        self.w = [up(a) for blk in c["blocks"] for a in blk]
        self.saved = torch.full((self.engine_call(e, "saved_bytes")(shape),), 0xFF, dtype=torch.uint8, device="cuda")
        self.y = nan(*y_shape)
        self.g_x = nan(*self.x.shape)
        self.g_w = [None if a is None else nan(*a.shape) for a in self.w]
        torch_done()

    def engine_call(self, e, what):
        return getattr(e, "%s_%s" % (self.CALLS, what))

    def forward(self, e):
        self.engine_call(e, "forward_device")(self.shape, P(self.x), [P(a) for a in self.w], P(self.saved), P(self.y))

    def backward(self, e, want_g_x=True):
        self.engine_call(e, "backward_device")(self.shape, P(self.saved), [P(a) for a in self.w], P(self.g_y), P(self.g_x) if want_g_x else None,
                                               [P(a) for a in self.g_w])

    def dense(self, e, shapes):
        """shapes = {index: shape} -> [saved tensor `index` as a dense device tensor], through unpack_device into NaN-filled buffers."""
        out = [nan(*shape) for shape in shapes.values()]
        torch_done()
        for i, a in zip(shapes, out):
            self.engine_call(e, "unpack_device")(self.shape, P(self.saved), i, P(a))
        return out

    @classmethod
    def run(cls, e, c, want_g_x=True, **kw):
        """forward and backward of a fresh case -> its flat results"""
        d = cls(e, c, **kw)
        d.forward(e)
        d.backward(e, want_g_x)
        return d.results(e)

    def outputs(self):
        """-> [(name, tensor)]: what the calls write."""
        return [(self.NAMES[1], self.y), (self.NAMES[3], self.g_x), ("d_saved", self.saved)] + \
               [("g_w%d" % i, a) for i, a in enumerate(self.g_w) if a is not None]

    def inputs(self, c):
        """-> [(name, tensor, its values in the case)]"""
        return [(self.NAMES[0], self.x, c[self.NAMES[0]]), (self.NAMES[2], self.g_y, c[self.NAMES[2]])] + \
               [("w%d" % i, a, src) for i, (a, src) in enumerate(zip(self.w, [a for blk in c["blocks"] for a in blk])) if a is not None]


class TrunkDev(ChainDev):
    """A trunk case (trunk_cases) on the device."""
    CALLS, NAMES = "trunk", ("x", "y", "g_y", "g_x")

    def __init__(self, e, c, pool=None):
        n, h, w, cin, blocks, p = c["shape"]
        shape = (n, h, w, cin, blocks, p if pool is None else pool)
        super().__init__(e, c, shape, T.y_shape(shape))

    def unpack(self, e):
        """-> (t, out): lists of dense device tensors."""
        n, h, w = self.shape[:3]
        d = self.dense(e, {1 + j: (n, cout, h, w) for i, (cout, _) in enumerate(self.shape[4]) for j in (2 * i, 2 * i + 1)})
        return d[0::2], d[1::2]

    def results(self, e, ts=None, outs=None):
        """Everything the calls produced, flat like trunk_cases.flat (g_x the untouched NaN buffer if it was not asked for)."""
        if ts is None:
            ts, outs = self.unpack(e)
        x0, = self.dense(e, {0: self.x.shape})
        e.synchronize()
        r = T.flat({"y": num(self.y), "g_x": num(self.g_x), "t": [num(a) for a in ts], "out": [num(a) for a in outs],
                    "g_w": [tuple(num(a) for a in self.g_w[3 * i:3 * i + 3]) for i in range(len(ts))]})
        r["x"] = num(x0)
        return r


class TailDev(ChainDev):
    """A QT tail's case (qtail_cases) on the device."""
    CALLS, NAMES = "qtail", ("x4", "x9", "g_x9", "g_x4")
    WKEYS = [("%s_%d" % (nm, i), 3 * i + j) for i in range(4) for j, nm in enumerate(("g_w0", "g_w2", "g_wsc")) if (i, j) != (2, 2)]

    def __init__(self, e, c):
        n, h, w = c["shape"]
        super().__init__(e, c, c["shape"], (n, 8, h // 2, w // 2))

    def unpack(self, e):
        n, h, w = self.shape
        return self.dense(e, {i: (n, ch, h, w) if i < 7 else (n, 8, h // 2, w // 2) for i, ch in enumerate((64, 32, 32, 32, 32, 32, 32, 8, 8))})

    def results(self, e):
        """Everything the calls produced, flat like qtail_cases.flat (g_x4 the untouched NaN buffer if it was not asked for)."""
        s = self.unpack(e)
        e.synchronize()
        d = {"x9": num(self.y), "g_x4": num(self.g_x)}
        d.update({"s%d" % i: num(a) for i, a in enumerate(s)})
        d.update({k: num(self.g_w[j]) for k, j in self.WKEYS})
        return d


run_trunk = TrunkDev.run


def chain(e, c, ts_in, outs_in):
    """The trunk as block calls: forward block by block, y by torch; backward block by block on the GIVEN t_i and out_i -> flat
    results."""
    n, h, w = c["shape"][:3]
    pool = c["shape"][5]
    x = up(c["x"])
    ws = [tuple(up(a) for a in blk) for blk in c["blocks"]]
    ts, outs, xs = [], [], [x]
    for (ci, co, k), (w0, w2, wsc) in zip(T.block_shapes(c["shape"]), ws):
        t, out = nan(n, co, h, w), nan(n, co, h, w)
        torch_done()
        e.resblock_forward_device((n, h, w, ci, co, k), P(xs[-1]), P(w0), P(w2), P(wsc), P(t), P(out))
        ts.append(t); outs.append(out); xs.append(out)
    e.synchronize()
    y = F.max_pool2d(outs[-1], 2) if pool else outs[-1]
    g = up(c["g_y"])
    if pool:
        o = outs_in[-1].detach().clone().requires_grad_()
        g, = torch.autograd.grad(F.max_pool2d(o, 2), o, g)
        g = g.contiguous()
    torch_done()
    g_w = [None] * len(ws)
    for i in range(len(ws) - 1, -1, -1):
        ci, co, k = T.block_shapes(c["shape"])[i]
        w0, w2, wsc = ws[i]
        x_i = x if i == 0 else outs_in[i - 1]
        g_x, gw = nan(n, ci, h, w), tuple(None if a is None else nan(*a.shape) for a in ws[i])
        torch_done()
        e.resblock_backward_device((n, h, w, ci, co, k), P(x_i), P(ts_in[i]), P(outs_in[i]), P(w0), P(w2), P(wsc), P(g), P(g_x), P(gw[0]), P(gw[1]),
                                   P(gw[2]))
        g_w[i], g = gw, g_x
    e.synchronize()
    return T.flat({"y": num(y), "g_x": num(g), "t": [num(a) for a in ts], "out": [num(a) for a in outs],
                   "g_w": [tuple(num(a) for a in gw) for gw in g_w]})


# ---- a stem: pmp_stem_forward_device / pmp_stem_backward_device
class StemDev:
    """A stem case on the device: x inside a NaN-filled allocation, 37 words from its start; NaN-filled outputs (y: the given one)."""
    GUARD = 37

    def __init__(self, c, y=None):
        self.shape = c["shape"]
        n, h, w, cin, k, split = self.shape
        size = c["x"].size
        self.buf = nan(size + 2 * self.GUARD)
        self.x = self.buf[self.GUARD:self.GUARD + size].view(c["x"].shape)
        self.x.copy_(up(c["x"]))
        self.w, self.b, self.g_y = [up(a) for a in c["w"]], [up(a) for a in c["b"]], up(c["g_y"])
        self.y = nan(n, 32, h, w) if y is None else up(y)
        self.g_x = nan(*c["x"].shape)
        self.g_w, self.g_b = [nan(*a.shape) for a in c["w"]], [nan(*a.shape) for a in c["b"]]
        torch_done()

    def forward(self, e):
        e.stem_forward_device(self.shape, P(self.x), [P(a) for a in self.w], [P(a) for a in self.b], P(self.y))

    def backward(self, e, want_g_x=True):
        e.stem_backward_device(self.shape, P(self.x), P(self.y), [P(a) for a in self.w], P(self.g_y), P(self.g_x) if want_g_x else None,
                               [P(a) for a in self.g_w], [P(a) for a in self.g_b])

    def results(self, e):
        e.synchronize()
        assert torch.isnan(self.buf[:self.GUARD]).all() and torch.isnan(self.buf[-self.GUARD:]).all()
        return S.flat({"y": num(self.y), "g_x": num(self.g_x), "g_w": [num(a) for a in self.g_w], "g_b": [num(a) for a in self.g_b]})

    def outputs(self):
        """-> [(name, tensor)]: what the calls write."""
        return [("y", self.y), ("g_x", self.g_x)] + [("g_w%d" % i, a) for i, a in enumerate(self.g_w)] + [("g_b%d" % i, a) for i, a in enumerate(self.g_b)]

    def inputs(self, c):
        """-> [(name, tensor, its values in the case)]"""
        return [("x", self.x, c["x"]), ("g_y", self.g_y, c["g_y"])] + [("w%d" % i, a, src) for i, (a, src) in enumerate(zip(self.w, c["w"]))] + \
               [("b%d" % i, a, src) for i, (a, src) in enumerate(zip(self.b, c["b"]))]


def run_stem(e, c, want_g_x=True, y=None):
    """forward (unless the backward pass is GIVEN y) and backward -> flat results."""
    d = StemDev(c, y)
    if y is None:
        d.forward(e)
    d.backward(e, want_g_x)
    return d.results(e)


# ---- a head: pmp_head_forward_device / pmp_head_backward_device
class HeadDev:
    """A head case on the device: its inputs as .d, NaN-filled outputs as .o (att and g_q only with an attention input).  off4: every
    tensor 4 bytes behind a 16-byte boundary inside one NaN-patterned allocation each (Off4)."""
    IN_F, IN_B = ("x", "w", "b", "prev", "q"), ("x", "w", "g_y", "g_att")
    OUT_F, OUT_B = ("y", "att"), ("g_x", "g_w", "g_b", "g_q", "g_prev")

    def __init__(self, c, off4=False):
        self.c, self.shape = c, c["shape"]
        sz = H.sizes(self.shape)
        self.d = {k: up(c[k]) for k in set(self.IN_F + self.IN_B)}
        self.o = {k: nan(*sz[k]) for k in self.OUT_F + self.OUT_B if sz[k]}
        self.guards = []
        if off4:
            for group in (self.d, self.o):
                for k, t in group.items():
                    if t is not None:
                        self.guards.append(Off4(t))
                        group[k] = self.guards[-1].view
        torch_done()

    def forward(self, e):
        d, o = self.d, self.o
        e.head_forward_device(self.shape, P(d["x"]), P(d["w"]), P(d["b"]), P(d["prev"]), P(d["q"]), P(o["y"]), P(o.get("att")))

    def backward(self, e, want_g_x=None, want_g_q=None, want_g_prev=None):
        c, d, o = self.c, self.d, self.o
        pick = lambda flag, default, k: P(o.get(k)) if (default if flag is None else flag) else None
        e.head_backward_device(self.shape, P(d["x"]), P(d["w"]), P(d["g_y"]), P(d["g_att"]), pick(want_g_x, c["want_g_x"], "g_x"), P(o["g_w"]),
                               P(o["g_b"]), pick(want_g_q, c["want_g_q"], "g_q"), pick(want_g_prev, c["prev"] is not None, "g_prev"))

    def results(self, e):
        e.synchronize()
        assert all(g.guards_intact() for g in self.guards)
        return {k: num(v) for k, v in self.o.items()}

    def outputs(self):
        return list(self.o.items())

    def inputs(self):
        return [(k, t, self.c[k]) for k, t in self.d.items() if t is not None]


# ---- determinism: twice, on a second stream, on a second context
def same_bits_on_every_run_stream_and_context(eng, run, c, nonzero=False, context_stream=True):
    """run(engine, c) -> a dict of results: no NaN in it (nonzero: and no tensor all zero), and the same bits again, on a second
    stream and on a second context (context_stream: that one on a stream of torch's, otherwise on its own)."""
    from pmp_vvc_tip2023_amd import engine
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
        if context_stream:
            side2 = torch.cuda.Stream()
            e2.set_stream(side2.cuda_stream)
        runs["second context on another stream" if context_stream else "second context"] = run(e2, c)
    finally:
        e2.close()
    for what, r in runs.items():
        for k, v in first.items():
            assert not np.isnan(v).any() and same_bits(r[k], v), (what, k)
            assert not nonzero or np.abs(v).max() > 0, (what, k)


# ---- refusals: PMP_E_INVALID before any launch, nothing written
def refuse_all(eng, tries, call):
    """tries = [(what, case name, which call, keyword arguments of call)]: every one is refused with a message; then both streams
    are drained, so that a kernel a refused call had launched all the same would have written by the time the caller looks."""
    for what, nm, which, kw in tries:
        assert call(nm, which, **kw) == -1, (what, which)
        assert eng.lib.pmp_last_error(eng.h), what
    eng.synchronize()
    torch.cuda.synchronize()


def chain_refusal_call(eng, variant, pick, dense):
    """-> call(nm, what, ...) of a chain's refusal test, through the C ABI: "forward", "backward" or "unpack" of pick(nm, what), a
    TrunkDev or TailDev (variant: its class), the keyword arguments replacing what the call passes: shape (null_shape: none), w and g_w
    {position in the array: pointer} (null_w, null_g_w: no array), index, and by name x, y, g_y, g_x (as in NAMES), saved and dense."""
    from pmp_vvc_tip2023_amd import _lib
    x, y, g_y, g_x = variant.NAMES
    arr = lambda ps: (C.c_void_p * len(ps))(*ps)
    fn = lambda what: getattr(eng.lib, "pmp_%s_%s_device" % (variant.CALLS, what))

    def call(nm, what, shape=None, null_shape=False, w=None, g_w=None, null_w=False, null_g_w=False, index=1, **swap):
        d = pick(nm, what)
        p = {x: P(d.x), "saved": P(d.saved), y: P(d.y), g_y: P(d.g_y), g_x: P(d.g_x), "dense": P(dense)}
        p.update(swap)
        ws, gws = [P(a) for a in d.w], [P(a) for a in d.g_w]
        for i, v in (w or {}).items():
            ws[i] = v
        for i, v in (g_w or {}).items():
            gws[i] = v
        s = getattr(_lib, variant.CALLS + "_shape")(shape or d.shape)
        sp = None if null_shape else C.byref(s)
        wa, ga = None if null_w else arr(ws), None if null_g_w else arr(gws)
        if what == "forward":
            return fn(what)(eng.h, sp, p[x], wa, p["saved"], p[y])
        if what == "backward":
            return fn(what)(eng.h, sp, p["saved"], wa, p[g_y], p[g_x], ga)
        return fn(what)(eng.h, sp, p["saved"], index, p["dense"])
    return call


def check_untouched(nm, outputs, inputs, skip=()):
    """outputs = [(name, tensor)] not in skip still hold what they were filled with (NaN; a uint8 d_saved 0xFF bytes), and inputs =
    [(name, tensor, values)] still hold the case's bits."""
    for k, a in outputs:
        if k in skip:
            continue
        if a.dtype == torch.uint8:
            assert (a == 0xFF).all(), (nm, k, "written by a refused call")
        else:
            assert torch.isnan(a).all(), (nm, k, "written by a refused call")
    for k, a, src in inputs:
        assert same_bits(a.cpu().numpy(), src), (nm, k, "an input changed")
