"""The plane scan's line context of a candidate (region_line_context: the '\\n'
count before it and the start of its line, from the finding thread's 64-byte
'\\n' mask, its block-scan prefix and the last '\\n' before its region) against
a byte-by-byte model on the host, and the identity "context at q = context at
the window start" for every valid window at k 5, 16, 32 and 64
(tests/native/scan_line_context_check.hip, built with hipcc from the library's
own header; no GPU needed)."""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
HIPCC = "/opt/rocm/bin/hipcc"


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_region_line_context_matches_the_byte_model(tmp_path):
    exe = tmp_path / "scan_line_context_check"
    src = os.path.join(HERE, "native", "scan_line_context_check.hip")
    inc = os.path.join(HERE, "..", "kmerjs_amd", "csrc")
    subprocess.run([HIPCC, "-O2", "-std=c++17", "-I", inc, "-o", str(exe), src], check=True,
                   capture_output=True, timeout=300)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert " 0 of " in r.stdout
