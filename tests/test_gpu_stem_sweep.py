"""GPU: the stem's forward and backward over the shapes include/pmp.h accepts - the table of tests/stem_sweep_cases.py, whose reach
tests/test_stem_sweep_cpu.py asserts: all sixteen (cin, k, split) at two shapes, sides and n of 256, the cap of the reduction's
partition with the wide accumulator sets, masks on the edge of `> 0`, subnormals made and consumed by the kernels, every tensor of a
call 4 bytes off a 16-byte boundary between guard words or touching its neighbours, float cases with a real second-stage chain, and
stem.py on the tensors a trainer passes.

Bounds.  EXACT, MASK_EDGES and TINY cases: every output equals the float64 restatement BIT FOR BIT, no element left out, into
NaN-filled outputs in workspaces poisoned with pattern 2 (tests/test_gpu_stem_grad.py keeps both patterns on its own table), once
without g_x.  FLOAT cases: every element within |gpu - ref64| <= c * 2^-24 * A + 2^-23 * |ref64| with stem_sweep_cases' constants;
`pytest -s` prints the largest ratio per kernel, recorded in stem_sweep_cases.GPU_RATIOS.  stem.py: bit-equal to its own call on
contiguous float32 tensors."""
import numpy as np
import pytest
import torch

import stem_cases as S
import stem_sweep_cases as W
import train_rig as R

pytestmark = pytest.mark.gpu
Dev, run, check_bits = R.StemDev, R.run_stem, R.check_bits_same_keys
RATIOS = {}
PATTERN = 0x7FC5A5A5                               # a quiet NaN with a payload nothing computes
eng = R.engine_fixture(poison=2)


# ---- 1. every exact case of the table
@pytest.mark.parametrize("name", list(W.EXACT))
def test_exact_cases_bit_equal(eng, name):
    c, want = W.exact(name)
    check_bits(name, run(eng, c), want)
    got = run(eng, c, want_g_x=False)
    assert np.isnan(got["g_x"]).all()
    check_bits(name + " without g_x", got, want, skip=("g_x",))


# ---- 2. masks on the edge of `> 0`; subnormals
@pytest.mark.parametrize("name", list(W.MASK_EDGES))
def test_mask_edges_bit_equal(eng, name):
    c, y, want = W.mask_edges(name)
    check_bits(name, run(eng, c, y=y), want)


@pytest.mark.parametrize("which", ["x_tiny", "g_tiny"])
@pytest.mark.parametrize("name", list(W.TINY))
def test_tiny_cases_bit_equal(eng, name, which):
    """x_tiny: the forward kernel makes the subnormal y that the three masks of the backward pass then compare."""
    c, want, _ = W.tiny(name, which)
    got = run(eng, c)
    for key in W.scaled_outputs(c, which):
        flushed = (want[key] != 0) & (got[key] == 0)
        assert not flushed.any(), (name, which, key, "%d subnormal results flushed to zero" % flushed.sum())
    check_bits("%s %s" % (name, which), got, want)


# ---- 3. every tensor of a call in ONE allocation: 4 (or 12) bytes off a 16-byte boundary between guard words, or touching
class Arena(Dev):
    """Every tensor of a call a view of one allocation filled with PATTERN.  guard words between neighbours, each view `first` words
    past a 16-byte boundary; guard None: back to back, nothing in between.  Order: x, y, then w, g_w, g_b, b per convolution, g_y, g_x - every
    output lies right behind a tensor of the call that writes it."""
    LEAD, TAIL = 36, 37

    def __init__(self, c, first=1, guard=33):
        self.shape = c["shape"]
        n, h, w, cin, k, split = self.shape
        nc = len(c["w"])
        shapes = [("x", c["x"].shape), ("y", (n, 32, h, w))]
        for j in range(nc):
            shapes += [("w%d" % j, c["w"][j].shape), ("g_w%d" % j, c["w"][j].shape), ("g_b%d" % j, c["b"][j].shape), ("b%d" % j, c["b"][j].shape)]
        shapes += [("g_y", (n, 32, h, w)), ("g_x", c["x"].shape)]
        self.at, off = {}, self.LEAD
        for i, (nm, shp) in enumerate(shapes):
            size = int(np.prod(shp))
            start = off + (first if i == 0 else 0) if guard is None else (off + guard + 3) // 4 * 4 + first
            assert guard is None or (start - off >= guard and start % 4 == first)
            self.at[nm] = (start, size, tuple(shp))
            off = start + size
        self.words = off + self.TAIL
        self.bits = torch.full((self.words,), PATTERN, dtype=torch.int32, device="cuda")
        self.buf = self.bits.view(torch.float32)
        assert self.buf.data_ptr() % 16 == 0
        view = lambda nm: self.buf[self.at[nm][0]:self.at[nm][0] + self.at[nm][1]].view(self.at[nm][2])
        self.x, self.y, self.g_y, self.g_x = view("x"), view("y"), view("g_y"), view("g_x")
        self.w, self.b = [view("w%d" % j) for j in range(nc)], [view("b%d" % j) for j in range(nc)]
        self.g_w, self.g_b = [view("g_w%d" % j) for j in range(nc)], [view("g_b%d" % j) for j in range(nc)]
        self.sources = dict([("x", c["x"]), ("g_y", c["g_y"])] + [("w%d" % j, a) for j, a in enumerate(c["w"])] +
                            [("b%d" % j, a) for j, a in enumerate(c["b"])])
        for nm, a in self.sources.items():
            view(nm).copy_(R.up(a))
        for t in [self.x, self.y, self.g_y, self.g_x] + self.w + self.b + self.g_w + self.g_b:
            assert t.data_ptr() % 4 == 0 and (guard is None or t.data_ptr() % 16 == 4 * first)
        R.torch_done()

    def outputs(self):
        return [nm for nm in self.at if nm not in self.sources]

    def host(self, e):
        e.synchronize()
        torch.cuda.synchronize()
        return self.bits.cpu().numpy().view(np.uint32)

    def piece(self, bits, nm):
        start, size, shp = self.at[nm]
        return bits[start:start + size].view(np.float32).reshape(shp)

    def results(self, e, untouched=()):
        """-> flat results; every word outside the call's tensors, and every tensor in `untouched`, still holds PATTERN; the inputs
        hold what was put there."""
        bits = self.host(e)
        free = np.ones(self.words, bool)
        for nm, (start, size, _) in self.at.items():
            if nm not in untouched:
                free[start:start + size] = False
        bad = np.flatnonzero(free & (bits != PATTERN))
        assert bad.size == 0, ("words outside the outputs were written", bad[:8], [(nm, v[0], v[0] + v[1]) for nm, v in self.at.items()])
        for nm, a in self.sources.items():
            assert S.same_bits(self.piece(bits, nm), a), (nm, "an input was written")
        return {nm: self.piece(bits, nm).copy() for nm in self.outputs()}


@pytest.mark.parametrize("first", [1, 3])
@pytest.mark.parametrize("name", list(W.ARENA))
def test_every_tensor_off_16_bytes_between_guards(eng, name, first):
    c = S.make_case(name, shape=W.ARENA[name])
    want = {k: S.as_f32(v) for k, v in S.flat(S.restate(c)).items()}
    d = Arena(c, first=first, guard=33)
    d.forward(eng)
    check_bits(name + " forward", {"y": d.results(eng, untouched=[nm for nm in d.outputs() if nm != "y"])["y"]}, {"y": want["y"]})
    d.backward(eng)
    check_bits(name, d.results(eng), want)


@pytest.mark.parametrize("name", list(W.ARENA))
def test_touching_tensors_are_accepted_and_one_shared_word_is_refused(eng, name):
    from pmp_vvc_tip2023_amd import _lib
    c = S.make_case(name, shape=W.ARENA[name])
    want = {k: S.as_f32(v) for k, v in S.flat(S.restate(c)).items()}
    d = Arena(c, first=1, guard=None)
    order = list(d.at)
    for a, b in zip(order, order[1:]):
        assert d.at[a][0] + d.at[a][1] == d.at[b][0], "back to back"
    P = R.P
    ptr = {nm: d.buf.data_ptr() + 4 * v[0] for nm, v in d.at.items()}
    nc = len(c["w"])
    arr = lambda key, p: [p["%s%d" % (key, j)] for j in range(nc)]

    def forward(p):
        eng.stem_forward_device(d.shape, p["x"], arr("w", p), arr("b", p), p["y"])

    def backward(p):
        eng.stem_backward_device(d.shape, p["x"], p["y"], arr("w", p), p["g_y"], p["g_x"], arr("g_w", p), arr("g_b", p))

    def refused(call, nm):
        """the call with output nm one word down, into the last word of its neighbour"""
        with pytest.raises(_lib.PmpError) as err:
            call(dict(ptr, **{nm: ptr[nm] - 4}))
        assert err.value.code == -1 and "overlap" in str(err.value), (nm, str(err.value))

    assert P(d.x) == ptr["x"] and P(d.g_b[-1]) == ptr["g_b%d" % (nc - 1)]
    refused(forward, "y")
    assert sorted(d.results(eng, untouched=d.outputs())) == sorted(want), "a refused forward wrote nothing"
    forward(ptr)
    y = d.results(eng, untouched=[nm for nm in d.outputs() if nm != "y"])["y"]
    check_bits(name + " forward", {"y": y}, {"y": want["y"]})
    for nm in d.outputs():
        if nm != "y":
            refused(backward, nm)
    d.results(eng, untouched=[nm for nm in d.outputs() if nm != "y"])          # the refused backward calls wrote nothing
    backward(ptr)
    check_bits(name, d.results(eng), want)


# ---- 4. float values within the bound, every element
@pytest.mark.parametrize("name", list(W.FLOAT))
def test_float_cases_within_the_bound(eng, name):
    c, y32, ref, bound, A = W.float_reference(name)
    d = Dev(c)
    d.forward(eng)
    got = {"y": d.results(eng)["y"]}
    got.update({k: v for k, v in run(eng, c, y=y32).items() if k != "y"})
    assert sorted(got) == sorted(ref)
    worst = {}
    for k in ref:
        assert got[k].shape == ref[k].shape and np.isfinite(got[k]).all(), (name, k)
        r = S.ratio(got[k], ref[k], bound[k])
        worst[W.KERNEL_OF(k)] = max(worst.get(W.KERNEL_OF(k), 0.0), r)
    for kernel, r in worst.items():
        RATIOS[kernel] = max(RATIOS.get(kernel, 0.0), r)
        print("%-16s %-8s largest |gpu - ref64| / bound = %.3f   (so far: %.3f)" % (name, kernel, r, RATIOS[kernel]))
    for k in ref:
        r = S.ratio(got[k], ref[k], bound[k])
        assert r <= 1.0, (name, k, r)


# ---- 5. stem.py on what a trainer passes: bit-equal to its own call on contiguous float32 tensors
def _py_case(name):
    """-> (x, weights, biases, g_y): contiguous float32 on the device."""
    shape = W.STEM_PY[name]
    n, h, w, cin, k, split = shape
    g = torch.Generator().manual_seed(S._seed(name))
    rn = lambda *s: torch.randn(s, generator=g)
    x = rn(n, cin, h + k // 2, w + k // 2).cuda()
    ws = [(rn(*s) * (s[1] * s[2] * s[3]) ** -0.5).cuda() for s in S.conv_shapes(shape)]
    bs = [rn(s[0]).cuda() for s in S.conv_shapes(shape)]
    return x, ws, bs, rn(n, 32, h, w).cuda()


def _call(eng, x, ws, bs, backward, x_grad=True):
    """stem.stem on fresh leaves -> (flat results as numpy, x.grad as a tensor)."""
    from pmp_vvc_tip2023_amd import stem
    before = eng.stream_ptr
    x = x.detach().requires_grad_(x_grad)
    ws, bs = [t.clone().requires_grad_() for t in ws], [t.clone().requires_grad_() for t in bs]
    y = stem.stem(eng, x, list(zip(ws, bs)))
    backward(y)
    assert eng.stream_ptr == before, "the engine is back on the stream it was on"
    torch.cuda.synchronize()
    num = lambda t: t.detach().cpu().numpy()
    r = {"y": num(y), "g_w": [num(t.grad) for t in ws], "g_b": [num(t.grad) for t in bs], "g_x": num(x.grad.float())}
    for v in S.flat(r).values():
        assert np.isfinite(v).all() and np.abs(v).max() > 0
    return S.flat(r), x.grad


@pytest.mark.parametrize("name", list(W.STEM_PY))
def test_stem_py_takes_a_crop_and_a_float64_x(eng, name):
    x, ws, bs, g_y = _py_case(name)
    want, _ = _call(eng, x, ws, bs, lambda y: y.backward(g_y))
    n, cin, hx, wx = x.shape
    big = torch.randn((n, cin, hx + 7, wx + 9), generator=torch.Generator().manual_seed(5)).cuda()
    crop = big[:, :, 3:3 + hx, 5:5 + wx]
    crop.copy_(x)
    assert not crop.is_contiguous() and crop.shape == x.shape
    got, grad = _call(eng, crop, ws, bs, lambda y: y.backward(g_y))
    check_bits(name + " crop", got, want)
    assert grad.shape == crop.shape and grad.dtype == torch.float32
    got, grad = _call(eng, x.double(), ws, bs, lambda y: y.backward(g_y))
    check_bits(name + " float64 x", got, want)
    assert grad.shape == x.shape and grad.dtype == torch.float64 and torch.equal(grad, torch.from_numpy(want["g_x"]).cuda().double())


@pytest.mark.parametrize("name", list(W.STEM_PY))
def test_stem_py_takes_a_permuted_and_an_expanded_g_y(eng, name):
    x, ws, bs, g_y = _py_case(name)
    perm = g_y.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)             # the values of g_y, channels last in memory
    assert not perm.is_contiguous() and torch.equal(perm, g_y)
    want, _ = _call(eng, x, ws, bs, lambda y: y.backward(g_y))
    got, _ = _call(eng, x, ws, bs, lambda y: y.backward(perm))
    check_bits(name + " permuted g_y", got, want)
    want, _ = _call(eng, x, ws, bs, lambda y: y.backward(torch.ones_like(y)))
    got, _ = _call(eng, x, ws, bs, lambda y: y.sum().backward())
    check_bits(name + " y.sum().backward()", got, want)


@pytest.mark.parametrize("name", list(W.STEM_PY))
def test_stem_py_on_a_side_stream_without_host_synchronisation(eng, name):
    """The inputs are produced on the side stream right before the call, behind a matrix product that keeps that stream busy: a call
    that ran on another stream would read them before they exist."""
    from pmp_vvc_tip2023_amd import stem
    x, ws, bs, g_y = _py_case(name)
    want, _ = _call(eng, x, ws, bs, lambda y: y.backward(g_y))
    m = torch.full((4096, 4096), 2.0 ** -6, device="cuda")
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        m @ m                                      # the first product loads its library: not while the host is meant to run ahead
    torch.cuda.synchronize()
    before = eng.stream_ptr
    with torch.cuda.stream(side):
        busy = m @ m @ m
        zero = busy[0, 0] * 0
        xs = (x + zero).requires_grad_()
        wl, bl = [(t + zero).requires_grad_() for t in ws], [(t + zero).requires_grad_() for t in bs]
        gs = g_y + zero
        y = stem.stem(eng, xs, list(zip(wl, bl)))
        y.backward(gs)
    assert eng.stream_ptr == before, "the engine's stream is restored"
    side.synchronize()
    num = lambda t: t.detach().cpu().numpy()
    got = S.flat({"y": num(y), "g_x": num(xs.grad), "g_w": [num(t.grad) for t in wl], "g_b": [num(t.grad) for t in bl]})
    assert S.same_bits(num(xs), num(x)) and float(zero) == 0.0
    check_bits(name + " side stream", got, want)
