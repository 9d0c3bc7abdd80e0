"""ORACLE (test infrastructure, not product): reading the GPU's tensor taps (pmp_debug_set_taps / pmp_debug_get_tap, include/pmp.h).

Shared by the layer-local tests (tests/test_gpu_layers.py) and the site-by-site range tests (tests/test_gpu_range_sites.py)."""
import ctypes as C

import numpy as np


def taps_on(e, on):
    """Record (on) or stop recording and free (off) every intermediate tensor of an Engine's inference calls."""
    e._ck(e.lib.pmp_debug_set_taps(e.h, 1 if on else 0))


def tap(e, name):
    """-> (float64 [n, C padded, H, W] at true scale, real channel count); None if the last call has no such tensor."""
    dims, cr = (C.c_int * 4)(), C.c_int()
    n = e.lib.pmp_debug_get_tap(e.h, name.encode(), None, 0, dims, C.byref(cr))
    if n < 0:
        return None
    out = np.empty(int(n), np.float64)
    assert e.lib.pmp_debug_get_tap(e.h, name.encode(), out.ctypes.data_as(C.c_void_p), n, dims, C.byref(cr)) == n
    return out.reshape(tuple(dims)), cr.value
