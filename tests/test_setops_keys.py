"""The arithmetic of the long-pair join of kmer_setops.hip (the split depth, the
range of a remainder, the order of the ranges and the slot hash, all
__host__ __device__ helpers of kmer_internal.hpp) as a host model: it ends, and
its intersection, A-only and B-only sets equal a std::set join for remainder
sets of 0 .. 5 x JOIN_TILE entries -- uniform, with equal top bits, narrow,
identical and disjoint (tests/native/setops_keys_check.hip, built with hipcc
from the library's own header; no GPU needed)."""
import os
import re
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
HIPCC = "/opt/rocm/bin/hipcc"


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_host_model_of_the_join_equals_a_set_join(tmp_path):
    exe = tmp_path / "setops_keys_check"
    src = os.path.join(HERE, "native", "setops_keys_check.hip")
    inc = os.path.join(HERE, "..", "kmerjs_amd", "csrc")
    subprocess.run([HIPCC, "-O2", "-std=c++17", "-I", inc, "-o", str(exe), src], check=True,
                   capture_output=True, timeout=300)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    m = re.search(r"setops join: 0 of (\d+) mismatches", r.stdout)
    assert m and int(m.group(1)) >= 3 * 36 * 2, r.stdout
