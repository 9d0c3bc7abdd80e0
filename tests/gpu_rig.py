"""What the GPU test files share besides the yardstick (oracle/parity.py): the module's engine, as a context manager and as a fixture.
A plain module: every test file keeps the fixture name `eng`, its own cases and bounds."""
import contextlib
import os

import pytest

DATAPATHS = ("f16x3", "bf16x6", "fp32")


@contextlib.contextmanager
def engine(datapath=None, synthetic_mtt=False, poison=0, setup=None, threads=None):
    """An Engine on device 0 for the `with` block: `threads` caps torch's CPU threads (the float64 references), `datapath` selects the
    convolution datapath, `poison` fills its workspaces with that pattern from the start (and lifts it at the end), setup(e) makes the
    file's own calls (taps, fusion off, a saturation policy)."""
    import torch
    from pmp_vvc_tip2023_amd import engine as E
    assert torch.cuda.is_available()
    if threads:
        torch.set_num_threads(min(threads, os.cpu_count() or 1))
    e = E.Engine(0, allow_synthetic_mtt=synthetic_mtt)
    if datapath:
        e.set_precision(datapath)
        assert e.get_precision() == datapath
    if setup:
        setup(e)
    if poison:
        e._ck(e.lib.pmp_debug_poison_workspace(e.h, poison))
    try:
        yield e
        if poison:
            e._ck(e.lib.pmp_debug_poison_workspace(e.h, 0))
    finally:
        e.close()


def engine_fixture(datapaths=None, **how):
    """-> a module-scoped fixture: an engine() of the module's own, once per datapath of `datapaths` (the param ids are their names)."""
    def eng(request):
        with engine(getattr(request, "param", None), **how) as e:
            yield e
    return pytest.fixture(scope="module", params=datapaths)(eng)
