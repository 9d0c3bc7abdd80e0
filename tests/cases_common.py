"""What the training calls' case tables share (resblock_cases, grad_cases, stem_cases import these names): a float64 result as the
float32 a kernel must produce, bit equality of float32 tensors, and the largest error of a tensor in units of its bound; and what the
CPU tests of the tables hold against the built library: its kernel symbols."""
import os
import re
import shutil
import subprocess
import tempfile

import numpy as np
import pytest

ROCM_LLVM = "/opt/rocm/llvm/bin"
LIB = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "pmp_vvc_tip2023_amd", "libpmp_hip.so")


def kernel_symbols(lib, pattern):
    """{"conv_h2_kernel<3,3,4,0,1>", ...}: the kernel symbols of the gfx950 code objects bundled in `lib` that match `pattern` (group 1:
    the kernel's name, group 2: its mangled template arguments, absent for a kernel that is no template)."""
    objdump, readelf = os.path.join(ROCM_LLVM, "llvm-objdump"), os.path.join(ROCM_LLVM, "llvm-readelf")
    if not (os.path.exists(objdump) and os.path.exists(readelf)):
        pytest.skip("ROCm's llvm-objdump / llvm-readelf are not installed")
    out = set()
    d = tempfile.mkdtemp()
    try:
        copy = os.path.join(d, "lib.so")
        shutil.copy(lib, copy)                  # --offloading writes the extracted bundles next to its input
        subprocess.run([objdump, "--offloading", copy], cwd=d, check=True, capture_output=True)
        for f in os.listdir(d):
            if "amdgcn" not in f:
                continue
            syms = subprocess.run([readelf, "-W", "--syms", os.path.join(d, f)], check=True, capture_output=True, text=True).stdout
            for m in pattern.finditer(syms):
                out.add("%s<%s>" % (m.group(1), ",".join(re.findall(r"L[ib](\d+)E", m.group(2)))) if m.group(2) else m.group(1))
    finally:
        shutil.rmtree(d)
    return out


def as_f32(a):
    """A float64 result as the float32 a kernel must produce: rounded once, zeros positive (a kernel's sums start from +0)."""
    return None if a is None else (np.asarray(a, np.float64) + 0.0).astype(np.float32)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def ratio(got, ref, bound):
    """max |got - ref| / bound over a tensor (0 / 0 = 0; a difference where the bound is 0 is inf)."""
    d = np.abs(np.asarray(got, np.float64) - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        return float(np.where(d == 0, 0.0, d / bound).max())
