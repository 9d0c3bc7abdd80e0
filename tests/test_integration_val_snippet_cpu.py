"""CPU: the C block of INTEGRATION.md section 6 (validation, device-resident) compiles as plain C against include/pmp.h."""
import os
import re
import subprocess

from conftest import ROOT


def test_section6_c_block_compiles(tmp_path):
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    sec = text[text.index("## 6. Validating a pair of nets"):]
    blocks = re.findall(r"```c\n(.*?)```", sec, re.S)
    assert len(blocks) == 1 and "pmp_val_stats_device" in blocks[0] and "pmp_synchronize" in blocks[0]
    src = tmp_path / "val_snippet.c"
    src.write_text('#include "pmp.h"\n' + blocks[0])
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)])
