"""GPU: pmp_grad_pack_device and pmp_grad_sum_device (include/pmp.h, TRAINING STEP), in one process.  Nothing here has a tolerance.

Pack: tensors of 1, 3, 4, 5, 1023 and 65537 floats, one of them absent (NULL), every gradient once 16-byte aligned and once 4 bytes
behind such a boundary, and 97 tensors, which take two launches; the bucket is NaN beforehand and lies between NaN guards, so a float
the kernel does not write, or one it writes outside the bucket, shows.  Expected: grad_bucket_cases.packed, bit for bit.
Sum: 1, 2, 3 and 5 sources of 2404 floats (three workgroups, the last ragged), in place (d_dst = d_src[0]) and out of place, on values
whose float32 sum depends on the order (per element a permutation of 1e8, -1e8, 1, 2^-20; test_grad_sync_cpu.py asserts that the
reverse order gives other bits for 3 and 5 sources) against numpy float32 added in the same order: equal bits.  A larger sum of
2^21 + 4 floats covers the grid-stride loop (more quads than 2048 workgroups of 256 threads).
Both: the same bits on a second run, on another stream and on another context; the refusal table, with nothing written."""
import ctypes as C

import numpy as np
import pytest
import torch

import grad_bucket_cases as B
import train_rig as R
from cases_common import same_bits

pytestmark = pytest.mark.gpu
eng = R.engine_fixture()
GUARD = 64


class Guarded:
    """count floats between two NaN guards, NaN themselves; .view is 16-byte aligned"""

    def __init__(self, count):
        self.buf = R.nan(count + 2 * GUARD)
        self.view = self.buf[GUARD:GUARD + count]
        assert self.view.data_ptr() % 16 == 0

    def guards_intact(self):
        return bool(torch.isnan(self.buf[:GUARD]).all()) and bool(torch.isnan(self.buf[GUARD + self.view.numel():]).all())


def pack(e, counts, grads, off4=False):
    """grads: numpy arrays, None = absent -> the bucket's floats"""
    total, _ = B.layout(counts)
    dev = [None if g is None else (R.Off4(R.up(g)).view if off4 else R.up(g)) for g in grads]
    out = Guarded(total)
    R.torch_done()
    e.grad_pack_device([R.P(t) for t in dev], counts, R.P(out.view))
    e.synchronize()
    assert out.guards_intact()
    return R.num(out.view)


@pytest.mark.parametrize("off4", [False, True])
@pytest.mark.parametrize("absent", [None, 2, 5])
def test_pack_writes_every_float_of_the_bucket(eng, absent, off4):
    grads = B.gradients(B.COUNTS)
    if absent is not None:
        grads[absent] = None
    got = pack(eng, B.COUNTS, grads, off4)
    want = B.packed(grads, B.COUNTS)
    assert got.dtype == np.float32 and same_bits(got, want), np.argwhere(got.view(np.uint32) != want.view(np.uint32))[:4]
    assert not np.signbit(got[got == 0]).any(), "padding and absent slices are +0.0"


def test_pack_of_97_tensors_takes_two_launches(eng):
    grads = B.gradients(B.MANY, seed=12)
    grads[40] = None
    got = pack(eng, B.MANY, grads)
    assert same_bits(got, B.packed(grads, B.MANY))
    total, offsets = B.layout(B.MANY)
    assert np.array_equal(got[offsets[96]:offsets[96] + B.MANY[96]], grads[96]), "the tensor of the second launch"


def run_sum(e, src, in_place, count=None):
    count = src[0].size if count is None else count
    dev = [Guarded(count) for _ in src]
    for d, s in zip(dev, src):
        d.view.copy_(torch.from_numpy(s))
    out = dev[0] if in_place else Guarded(count)
    R.torch_done()
    e.grad_sum_device([R.P(d.view) for d in dev], count, R.P(out.view))
    e.synchronize()
    assert all(d.guards_intact() for d in dev + [out])
    for d, s in zip(dev[1:] if in_place else dev, src[1:] if in_place else src):
        assert same_bits(R.num(d.view), s), "a source changed"
    return R.num(out.view)


@pytest.mark.parametrize("in_place", [False, True])
@pytest.mark.parametrize("nsrc", B.NSRC)
def test_sum_adds_in_the_order_given(eng, nsrc, in_place):
    src = B.sources(nsrc)
    got = run_sum(eng, src, in_place)
    want = B.ordered_sum(src)
    assert got.dtype == np.float32 and same_bits(got, want), np.argwhere(got.view(np.uint32) != want.view(np.uint32))[:4]
    if nsrc > 2:
        assert not same_bits(got, B.ordered_sum(src[::-1])), "the reverse order gives other bits on these inputs"


def test_sum_of_more_quads_than_the_grid_has_threads(eng):
    src = B.sources(3, count=(1 << 21) + 4, seed=6)
    assert same_bits(run_sum(eng, src, True), B.ordered_sum(src))


def test_sum_keeps_signed_zeros_and_non_finite_values(eng):
    a = np.array([-0.0, -0.0, 0.0, np.inf, np.inf, np.nan, 1.0, -1.0], np.float32)
    b = np.array([-0.0, 0.0, -0.0, -np.inf, 1.0, 1.0, -1.0, 1.0], np.float32)
    got, want = run_sum(eng, [a, b], False), B.ordered_sum([a, b])
    nans = np.isnan(want)                                  # inf - inf and NaN + 1: a NaN's sign and payload are the hardware's
    assert nans.tolist() == [False, False, False, True, False, True, False, False] and np.array_equal(np.isnan(got), nans)
    assert same_bits(got[~nans], want[~nans]) and np.signbit(got[0]) and not np.signbit(got[1]) and not np.signbit(got[2]) and got[4] == np.inf
    assert same_bits(run_sum(eng, [a], False), a), "one source is a copy"


def test_the_same_bits_on_every_run_stream_and_context(eng):
    grads = B.gradients(B.COUNTS)
    grads[1] = None
    src = B.sources(5)

    def run(e, _):
        return {"bucket": pack(e, B.COUNTS, grads, off4=True), "sum": run_sum(e, src, False), "sum in place": run_sum(e, src, True)}
    R.same_bits_on_every_run_stream_and_context(eng, run, None)


def test_refusals_come_before_any_launch(eng):
    lib, h = eng.lib, eng.h
    counts = (1, 3, 4, 5, 1023)
    total, _ = B.layout(counts)
    grads = [R.up(g) for g in B.gradients(counts)]
    bucket = Guarded(total)
    src = [Guarded(64) for _ in range(3)]
    for s in src:
        s.view.fill_(1.0)
    dst = Guarded(64)
    R.torch_done()
    arr = lambda ps: (C.c_void_p * len(ps))(*ps)
    i64 = lambda v: (C.c_int64 * len(v))(*v)
    gp, bp = [R.P(g) for g in grads], R.P(bucket.view)
    sp, dp = [R.P(s.view) for s in src], R.P(dst.view)

    def pack_call(nt=5, g=gp, c=counts, b=bp, null_g=False, null_c=False):
        return lib.pmp_grad_pack_device(h, nt, None if null_g else arr(g), None if null_c else i64(c), b)

    def sum_call(nsrc=3, s=sp, count=64, d=dp, null_s=False):
        return lib.pmp_grad_sum_device(h, nsrc, None if null_s else arr(s), count, d)
    tries = [
        ("ntensors 0", lambda: pack_call(nt=0)), ("ntensors -1", lambda: pack_call(nt=-1)), ("no gradient array", lambda: pack_call(null_g=True)),
        ("no count array", lambda: pack_call(null_c=True)), ("no bucket", lambda: pack_call(b=None)),
        ("a count of 0", lambda: pack_call(c=(1, 3, 0, 5, 1023))), ("a count of 2^30", lambda: pack_call(c=(1, 3, 4, 1 << 30, 1023))),
        ("a bucket 4 bytes off", lambda: pack_call(b=bp + 4)), ("a gradient 2 bytes off", lambda: pack_call(g=gp[:4] + [gp[4] + 2])),
        ("a gradient inside the bucket", lambda: pack_call(g=gp[:4] + [bp + 16])),
        ("nsrc 0", lambda: sum_call(nsrc=0)), ("nsrc 65", lambda: sum_call(nsrc=65, s=sp * 22)), ("no source array", lambda: sum_call(null_s=True)),
        ("no destination", lambda: sum_call(d=None)), ("a null source", lambda: sum_call(s=[sp[0], None, sp[2]])),
        ("count 0", lambda: sum_call(count=0)), ("count 6", lambda: sum_call(count=6)), ("count -4", lambda: sum_call(count=-4)),
        ("a destination 4 bytes off", lambda: sum_call(d=dp + 4, count=60)), ("a source 8 bytes off", lambda: sum_call(s=[sp[0], sp[1] + 8, sp[2]], count=60)),
        ("the destination is the second source", lambda: sum_call(d=sp[1])), ("the destination partly over the first source", lambda: sum_call(d=sp[0] + 16, count=60)),
    ]
    for what, call in tries:
        assert call() == -1, what
        assert lib.pmp_last_error(h), what
    assert b"pmp_grad_sum_device" in lib.pmp_last_error(h)
    eng.synchronize()
    torch.cuda.synchronize()
    assert torch.isnan(bucket.buf).all() and torch.isnan(dst.buf).all(), "written by a refused call"
    assert all(bool((s.view == 1.0).all()) and s.guards_intact() for s in src)
    assert pack_call() == 0 and sum_call() == 0 and sum_call(d=sp[0]) == 0, "and the accepted calls run"
    eng.synchronize()
    assert same_bits(R.num(dst.view), np.full(64, 3.0, np.float32)) and same_bits(R.num(src[0].view), np.full(64, 3.0, np.float32))
