"""The key arithmetic of the table's by-value readers (kmer_table_spectrum /
kmer_table_extract*: from a table entry to its Map keys, tab_entry_keys, and
from a planar code to the matcher's 2-bit code, tab_planar_code2) agrees with
the string route of the host result for every k in 1..32, both modes
(tests/native/abundance_keys_check.hip, built with hipcc from the library's own
header; no GPU needed)."""
import os
import re
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
HIPCC = "/opt/rocm/bin/hipcc"


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_entry_keys_agree_with_the_string_route(tmp_path):
    exe = tmp_path / "abundance_keys_check"
    src = os.path.join(HERE, "native", "abundance_keys_check.hip")
    inc = os.path.join(HERE, "..", "kmerjs_amd", "csrc")
    subprocess.run([HIPCC, "-O2", "-std=c++17", "-I", inc, "-o", str(exe), src], check=True,
                   capture_output=True, timeout=300)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    m = re.search(r"abundance keys: 0 of (\d+) mismatches", r.stdout)
    assert m and int(m.group(1)) > 100_000, r.stdout
