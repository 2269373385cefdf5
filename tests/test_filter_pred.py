"""The read filter's predicate (filter_match in kmer_internal.hpp, the one the
mark kernel calls) against unsigned __int128 brute force on the host
(tests/native/filter_pred_check.hip, built with hipcc from the library's own
header; no GPU needed)."""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
HIPCC = "/opt/rocm/bin/hipcc"


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_filter_match_equals_128_bit_arithmetic(tmp_path):
    exe = tmp_path / "filter_pred_check"
    src = os.path.join(HERE, "native", "filter_pred_check.hip")
    inc = os.path.join(HERE, "..", "kmerjs_amd", "csrc")
    subprocess.run([HIPCC, "-O2", "-std=c++17", "-I", inc, "-o", str(exe), src], check=True,
                   capture_output=True, timeout=300)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert " 0 of " in r.stdout
