"""The arithmetic of the set operation whose result stays a table
(kmer_table_setop_into; kmer_setops.hip): the value a walk gives a class, the
class count behind it, the result's entry, the slot check of the write pass and
the running offset across the ranges of a long bucket and across UNION's two
walks -- all __host__ __device__ helpers of kmer_internal.hpp -- as a host
model: its count and write passes agree, and its entries and big list equal a
std::map join of the two Maps for the three operations
(tests/native/setop_into_check.hip, built with hipcc from the library's own
header; no GPU needed)."""
import os
import re
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
HIPCC = "/opt/rocm/bin/hipcc"


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_host_model_of_the_result_table_equals_a_map_join(tmp_path):
    exe = tmp_path / "setop_into_check"
    src = os.path.join(HERE, "native", "setop_into_check.hip")
    inc = os.path.join(HERE, "..", "kmerjs_amd", "csrc")
    subprocess.run([HIPCC, "-O2", "-std=c++17", "-I", inc, "-o", str(exe), src], check=True,
                   capture_output=True, timeout=300)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    m = re.search(r"setop into: 0 of (\d+) mismatches", r.stdout)
    assert m and int(m.group(1)) == 2 * 3 * 4 * 2, r.stdout
