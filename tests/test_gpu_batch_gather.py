"""GPU: pmp_batch_gather_device (include/pmp.h, TRAINING STEP) against its numpy restatement (tests/batch_cases.py), bit for bit.

A set of N = 7 blocks; batches of n = 1, 5 (one row twice) and 257 rows, luma and chroma; every output alone, the others NULL, and
all together.  Every source and every output sits inside a guarded allocation (0xFF bytes around the sources and the byte outputs, NaN
around the float outputs), 4 bytes behind a 16-byte boundary, and the guards are intact afterwards.  Indices -1 and N give rows of
zeros - had their rows been read, the 0xFF guards around the set would show - and raise bit 0 of the status word, which a clean call
leaves zero.  The same bits on a second run, a second stream and a second context; refusals leave every output as it was."""
import ctypes as C

import numpy as np
import pytest
import torch

import batch_cases as B
import train_rig as R

pytestmark = pytest.mark.gpu
eng = R.engine_fixture()
COMPS = {"Luma": False, "Chroma": True}


class Bytes4:
    """A byte tensor 4 bytes behind a 16-byte boundary inside an allocation of 0xFF bytes (a: its values, or a shape to leave 0xFF)."""

    def __init__(self, a):
        a = np.full(a, 0xFF, np.uint8) if isinstance(a, tuple) else np.ascontiguousarray(a).view(np.uint8)
        self.buf = torch.full((a.size + 36,), 0xFF, dtype=torch.uint8, device="cuda")
        self.view = self.buf[4:4 + a.size].view(a.shape)
        self.view.copy_(torch.from_numpy(a))
        assert self.buf.data_ptr() % 16 == 0 and self.view.data_ptr() % 16 == 4

    def guards_intact(self):
        return bool((self.buf[:4] == 0xFF).all()) and bool((self.buf[4 + self.view.numel():] == 0xFF).all())


@pytest.fixture(scope="module")
def dev_set():
    """The set on the device, once: {key: Bytes4}, and its values"""
    d = B.dataset()
    dev = {k: Bytes4(v) for k, v in d.items()}
    R.torch_done()
    return d, dev


def source(dev, chroma, **swap):
    from pmp_vvc_tip2023_amd import _lib
    p = {k: R.P(t.view) for k, t in dev.items()}
    if not chroma:
        p["u"] = p["v"] = None
    p.update(swap)
    return _lib.BatchSrc(p["y"], p["u"], p["v"], p["qt8"], p["msbt"], p["msdire"], swap.get("count", B.N))


class Outputs:
    """The outputs of n rows, guarded and filled with NaN / 0xFF, the index and a zeroed status word."""

    def __init__(self, index, chroma):
        n = len(index)
        self.n, self.index = n, torch.from_numpy(np.asarray(index, np.int64)).cuda()
        self.f = {"x": R.Off4(R.nan(*((n, 3, 34, 34) if chroma else (n, 1, 68, 68)))), "qt_f": R.Off4(R.nan(n, 1, 8, 8))}
        self.b = {"qt8": Bytes4((n, 8, 8)), "msbt": Bytes4((n, 3, 16, 16)), "msdire": Bytes4((n, 3, 16, 16))}
        self.status = torch.zeros(1, dtype=torch.int32, device="cuda")
        R.torch_done()

    def ptr(self, k):
        return R.P((self.f.get(k) or self.b[k]).view)

    def run(self, e, src, keys=B.KEYS):
        e.batch_gather_device(src, R.P(self.index), self.n, R.P(self.status), **{"d_" + k: self.ptr(k) for k in keys})

    def results(self, e):
        e.synchronize()
        assert all(g.guards_intact() for g in list(self.f.values()) + list(self.b.values()))
        out = {k: R.num(g.view) for k, g in self.f.items()}
        out.update({k: g.view.cpu().numpy() for k, g in self.b.items()})
        out["msdire"] = out["msdire"].view(np.int8)
        return out, int(self.status.item())

    def outputs(self):
        return [(k, g.view) for k, g in list(self.f.items()) + list(self.b.items())]


def check(got, want, keys):
    for k in B.KEYS:
        if k in keys:
            assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape and np.array_equal(got[k], want[k]), k
        elif got[k].dtype == np.float32:
            assert np.isnan(got[k]).all(), (k, "written though not asked for")
        else:
            assert (got[k].view(np.uint8) == 0xFF).all(), (k, "written though not asked for")


@pytest.mark.parametrize("comp", list(COMPS))
@pytest.mark.parametrize("which", list(B.indices()))
def test_every_output_alone_and_all_together_bit_equal(eng, dev_set, which, comp):
    d, dev = dev_set
    index = B.indices()[which]
    want, _ = B.gather(d, index, COMPS[comp])
    for keys in [B.KEYS] + [(k,) for k in B.KEYS]:
        o = Outputs(index, COMPS[comp])
        o.run(eng, source(dev, COMPS[comp]), keys)
        got, status = o.results(eng)
        check(got, want, keys)
        assert status == 0, "a clean call leaves a zeroed status word zero"
    assert all(g.guards_intact() for g in dev.values())


@pytest.mark.parametrize("comp", list(COMPS))
def test_indices_outside_the_set_give_zero_rows_and_the_status_bit(eng, dev_set, comp):
    d, dev = dev_set
    index = np.array([2, -1, B.N, 6, -2 ** 62, 2 ** 62], np.int64)
    want, flag = B.gather(d, index, COMPS[comp])
    o = Outputs(index, COMPS[comp])
    o.run(eng, source(dev, COMPS[comp]))
    got, status = o.results(eng)
    check(got, want, B.KEYS)
    assert flag == 1 and status == 1
    for k in B.KEYS:
        assert not got[k][[1, 2, 4, 5]].any() and got[k][[0, 3]].any(), k
    o.run(eng, source(dev, COMPS[comp]))                     # nothing but the OR writes the word: it stays up
    assert o.results(eng)[1] == 1


@pytest.mark.parametrize("comp", list(COMPS))
def test_same_bits_on_every_run_stream_and_context(eng, dev_set, comp):
    d, dev = dev_set

    def run(e, index):
        o = Outputs(index, COMPS[comp])
        o.run(e, source(dev, COMPS[comp]))
        return o.results(e)[0]
    R.same_bits_on_every_run_stream_and_context(eng, run, B.indices()["n257"])


def test_refusals_leave_the_outputs_untouched(eng, dev_set):
    from pmp_vvc_tip2023_amd import _lib
    d, dev = dev_set
    o = {c: Outputs(B.indices()["n5"], COMPS[c]) for c in COMPS}
    other = torch.zeros(64, dtype=torch.uint8, device="cuda")
    R.torch_done()

    def call(nm, which, src=None, null=(), n=None, index="index", status="status", keys=B.KEYS, **swap):
        out = o[nm]
        p = {k: out.ptr(k) if k in keys else None for k in B.KEYS}
        p.update({k: v for k, v in swap.items() if k in B.KEYS})
        dst = _lib.BatchDst(p["x"], p["qt_f"], p["qt8"], p["msbt"], p["msdire"])
        s = source(dev, COMPS[nm], **(src or {}))
        a = {"src": C.byref(s), "dst": C.byref(dst), "index": R.P(out.index), "status": R.P(out.status)}
        a["index"], a["status"] = (a[index] if isinstance(index, str) else index), (a[status] if isinstance(status, str) else status)
        for k in null:
            a[k] = None
        return eng.lib.pmp_batch_gather_device(eng.h, a["src"], a["index"], out.n if n is None else n, a["dst"], a["status"])

    x_l = o["Luma"].ptr("x")
    tries = [("null src", "Luma", "", dict(null=("src",))), ("null dst", "Luma", "", dict(null=("dst",))),
             ("null index", "Luma", "", dict(null=("index",))), ("null status", "Luma", "", dict(null=("status",))),
             ("count 0", "Luma", "", dict(src=dict(count=0))), ("n 0", "Luma", "", dict(n=0)), ("n too large", "Luma", "", dict(n=65537)),
             ("no y", "Luma", "", dict(src=dict(y=None))), ("u without v", "Chroma", "", dict(src=dict(v=None))),
             ("v without u", "Chroma", "", dict(src=dict(u=None))), ("no output", "Luma", "", dict(keys=())),
             ("qt_f without its source", "Luma", "", dict(src=dict(qt8=None), keys=("qt_f",))),
             ("qt8 without its source", "Luma", "", dict(src=dict(qt8=None), keys=("x", "qt8"))),
             ("msbt without its source", "Chroma", "", dict(src=dict(msbt=None))),
             ("msdire without its source", "Chroma", "", dict(src=dict(msdire=None))),
             ("a source off by two bytes", "Luma", "", dict(src=dict(y=R.P(dev["y"].view) + 2))),
             ("an output off by two bytes", "Luma", "", dict(x=x_l + 2)), ("an index off by four bytes", "Luma", "", dict(index=R.P(o["Luma"].index) + 4)),
             ("a status word off by two bytes", "Luma", "", dict(status=R.P(other) + 2)),
             ("two outputs overlap", "Luma", "", dict(qt_f=x_l + 16)), ("an output over the index", "Luma", "", dict(qt8=R.P(o["Luma"].index))),
             ("an output over the status word", "Luma", "", dict(qt8=R.P(o["Luma"].status))),
             ("an output over the set", "Luma", "", dict(qt8=R.P(dev["msbt"].view)))]
    R.refuse_all(eng, tries, call)
    for nm, out in o.items():
        R.check_untouched(nm, out.outputs(), [])
        assert int(out.status.item()) == 0
    for k, g in dev.items():
        assert g.guards_intact() and np.array_equal(g.view.cpu().numpy().view(d[k].dtype), d[k]), k
    assert eng.lib.pmp_batch_gather_device(None, None, None, 1, None, None) == -1
