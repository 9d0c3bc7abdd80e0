"""CPU: the divergence guard's flags of python -m pmp_vvc_tip2023_amd.train_qbd before anything touches the GPU, and the guard's
three calls in the ctypes table and the library's export list.  plan() refuses a --clipNorm that is negative or not finite and a
negative --maxSkipped with status 2; the parser's defaults leave the Trainer on the unguarded optimiser (the arguments optim.Adam
receives, with stand-ins for the nets: no GPU); the flags reach it as max_grad_norm and skip_nonfinite; the verdict on the counters."""
import fnmatch
import os
import re

import pytest
import torch

from conftest import ROOT
from pmp_vvc_tip2023_amd import _lib, optim, q_net, train_qbd as T

CALLS = ("pmp_grad_guard_scratch_bytes", "pmp_grad_guard_device", "pmp_adam_step_guarded_device")


def parse(*flags):
    return T.build_parser().parse_args(["--inputDir", "/nonexistent", "--outDir", "/nonexistent"] + list(flags))


@pytest.mark.parametrize("flags,needle", [(("--clipNorm", "-1"), "--clipNorm"), (("--clipNorm", "nan"), "--clipNorm"), (("--clipNorm", "inf"), "--clipNorm"),
                                          (("--clipNorm=-inf",), "--clipNorm"), (("--maxSkipped", "-1"), "--maxSkipped")])
def test_plan_refuses_bad_guard_flags_with_status_2(capsys, flags, needle):
    with pytest.raises(SystemExit) as e:
        T.plan(parse(*flags))
    assert e.value.code == 2
    err = capsys.readouterr().err
    assert err.startswith("train_qbd: ") and needle in err, err
    assert not torch.cuda.is_initialized()


def test_good_guard_flags_pass_on_to_the_next_check(capsys):
    for flags in (("--clipNorm", "0"), ("--clipNorm", "2.5", "--skipNonFinite", "--maxSkipped", "0"), ()):
        with pytest.raises(SystemExit):
            T.plan(parse(*flags))
        assert "--inputDir" in capsys.readouterr().err


def test_defaults_are_off():
    a = parse()
    assert (a.clipNorm, a.skipNonFinite, a.maxSkipped) == (0.0, False, 10) and T.guard_kwargs(a) == {} and T.EXIT_DIVERGED == 5


class _Net(torch.nn.Module):
    """Stands in for q_net.QNet on the CPU: one parameter, and it stays where it is"""

    def __init__(self, engine, luma):
        super().__init__()
        self.w = torch.nn.Parameter(torch.zeros(3))

    def to(self, *a, **k):
        return self


@pytest.mark.parametrize("flags,want", [((), {}), (("--clipNorm", "0"), {}), (("--clipNorm", "2.5"), {"max_grad_norm": 2.5}),
                                        (("--skipNonFinite",), {"skip_nonfinite": True}),
                                        (("--clipNorm", "1", "--skipNonFinite", "--maxSkipped", "3"), {"max_grad_norm": 1.0, "skip_nonfinite": True})])
def test_the_arguments_optim_adam_receives(monkeypatch, flags, want):
    seen = []

    class Adam:
        def __init__(self, engine, params, **kw):
            seen.append((engine, list(params), kw))

    monkeypatch.setattr(q_net, "QNet", _Net)
    monkeypatch.setattr(optim, "Adam", Adam, raising=False)
    engine = object()
    tr = T.Trainer(engine, parse(*flags), "Chroma", {}, 0)
    (e, params, kw), = seen
    assert e is engine and len(params) == 1 and kw == dict({"lr": 1e-3}, **want)
    assert tr.guarded == bool(want) and tr.taken is None
    assert not torch.cuda.is_initialized()


def test_the_verdict_on_the_counters():
    a = parse("--skipNonFinite", "--maxSkipped", "3")
    c = {"steps": 8, "skipped": 3, "clipped": 0, "run": 3, "max_run": 3, "max_norm": 2.0}
    assert T.diverged(a, 1, c, None) is None and T.diverged(a, 1, c, 5) is None
    msg = T.diverged(a, 1, dict(c, max_run=4), None)
    assert "epoch 1" in msg and "max_run 4" in msg and "skipped 3" in msg and "--maxSkipped 3" in msg
    msg = T.diverged(a, 7, c, 0)
    assert "epoch 7" in msg and "no step of the epoch was taken" in msg and "steps 8" in msg


def test_lib_declares_the_three_calls():
    for name in CALLS:
        assert name in _lib.SIGNATURES, name
    assert _lib.SIGNATURES[CALLS[0]][0] is _lib._I64 and len(_lib.SIGNATURES[CALLS[1]][1]) == 8 and len(_lib.SIGNATURES[CALLS[2]][1]) == 10
    import ctypes as C
    assert C.sizeof(_lib.GuardRecord) == 32 and C.sizeof(_lib.GuardState) == 48 and C.sizeof(_lib.GuardParams) == 16
    assert _lib.GuardRecord.action.offset == 28 and _lib.GuardRecord.coef.offset == 24


def test_the_header_declares_and_the_export_list_names_the_three_calls():
    header = open(os.path.join(ROOT, "include", "pmp.h")).read()
    exported = re.findall(r"global:\s*([^;]+);", open(os.path.join(ROOT, "pmp_vvc_tip2023_amd", "csrc", "exports.map")).read())
    patterns = [p.strip() for part in exported for p in part.split(";") if p.strip()]
    for name in CALLS:
        assert re.search(r"\b%s\(" % name, header), name
        assert any(fnmatch.fnmatchcase(name, p) for p in patterns), (name, patterns)
