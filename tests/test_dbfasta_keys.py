"""The keys of a window on the FASTA route to a template DB (dbf_window_keys:
the emitted 2-bit codes and their number, both modes, every k in 1..32,
prefixes of length 0, 1, 5 and k) against a brute-force string model on the
host (tests/native/dbfasta_keys_check.hip, built with hipcc from the library's
own header; no GPU needed)."""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
HIPCC = "/opt/rocm/bin/hipcc"


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_window_keys_match_the_string_model(tmp_path):
    exe = tmp_path / "dbfasta_keys_check"
    src = os.path.join(HERE, "native", "dbfasta_keys_check.hip")
    inc = os.path.join(HERE, "..", "kmerjs_amd", "csrc")
    subprocess.run([HIPCC, "-O2", "-std=c++17", "-I", inc, "-o", str(exe), src], check=True,
                   capture_output=True, timeout=300)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert " 0 of " in r.stdout
