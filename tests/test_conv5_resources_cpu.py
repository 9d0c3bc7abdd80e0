"""The register budget of the 5x5 Cout-64 convolution kernels, read from the kernel descriptors' metadata in the built library (no GPU
needed): every conv_h2_kernel instantiation with KH = 5 and Cout = 64 that launch_h2 can reach (oracle/conv_cases.py: INSTANTIATIONS marked
reachable) fits three workgroups per CU - at most 168 VGPRs - without a spilled register or a byte of scratch.  Metadata only
(llvm-readelf --notes of the uncompressed code-object bundles, extracted as cases_common.kernel_symbols does); no instruction text.

The three kernels: <5,5,4,0,1> (no shortcut source), <5,5,4,2,0> (the 32-channel LDS shortcut) and <5,5,4,1,0> (a shortcut source of any
other width, tile by tile through LDS as well): 168 VGPRs each."""
import os
import re
import shutil
import subprocess
import tempfile

import pytest

from cases_common import LIB, ROCM_LLVM
from oracle import conv_cases as CC

KERNELS = sorted(k for k, why in CC.INSTANTIATIONS.items() if why is None and k.startswith("conv_h2_kernel<5,5,4,"))
_NAME = re.compile(r"_ZN3pmp\d+(conv_h2_kernel)I((?:L[ib]\d+E)+)E")


@pytest.fixture(scope="module")
def resources():
    """{"conv_h2_kernel<5,5,4,0,1>": {".vgpr_count": 168, ...}, ...} for every conv_h2_kernel in the library's gfx950 code objects."""
    objdump, readelf = os.path.join(ROCM_LLVM, "llvm-objdump"), os.path.join(ROCM_LLVM, "llvm-readelf")
    if not (os.path.exists(objdump) and os.path.exists(readelf)):
        pytest.skip("ROCm's llvm-objdump / llvm-readelf are not installed")
    out = {}
    d = tempfile.mkdtemp()
    try:
        copy = os.path.join(d, "lib.so")
        shutil.copy(LIB, copy)
        subprocess.run([objdump, "--offloading", copy], cwd=d, check=True, capture_output=True)
        for f in os.listdir(d):
            if "amdgcn" not in f:
                continue
            notes = subprocess.run([readelf, "--notes", os.path.join(d, f)], check=True, capture_output=True, text=True).stdout
            for entry in re.split(r"\n\s*- (?=\.\w+:)", notes):          # one list item per kernel under amdhsa.kernels
                name = re.search(r"\.name:\s+(\S+)", entry)
                m = _NAME.match(name.group(1)) if name else None
                if not m or ".vgpr_count" not in entry:
                    continue
                key = "%s<%s>" % (m.group(1), ",".join(re.findall(r"L[ib](\d+)E", m.group(2))))
                out[key] = {k: int(v) for k, v in re.findall(r"(\.\w+):\s+(\d+)\s*$", entry, re.M)}
    finally:
        shutil.rmtree(d)
    return out


def test_the_table_names_the_three_reachable_kernels():
    assert KERNELS == ["conv_h2_kernel<5,5,4,0,1>", "conv_h2_kernel<5,5,4,1,0>", "conv_h2_kernel<5,5,4,2,0>"]


@pytest.mark.parametrize("kernel", KERNELS)
def test_kernel_fits_three_workgroups_without_spills(resources, kernel):
    assert kernel in resources, sorted(resources)
    r = resources[kernel]
    print(kernel, {k: r[k] for k in (".vgpr_count", ".vgpr_spill_count", ".private_segment_fixed_size", ".sgpr_count")})
    assert r[".vgpr_spill_count"] == 0 and r[".private_segment_fixed_size"] == 0 and r[".vgpr_count"] <= 168, r
