"""The read screen's window arithmetic (planes -> codes -> h, and the weight of
a window in both modes, for every k in 1..32) against a brute-force string
model on the host (tests/native/screen_keys_check.hip, built with hipcc from
the library's own header; no GPU needed)."""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
HIPCC = "/opt/rocm/bin/hipcc"


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_screen_weight_and_h_match_the_string_model(tmp_path):
    exe = tmp_path / "screen_keys_check"
    src = os.path.join(HERE, "native", "screen_keys_check.hip")
    inc = os.path.join(HERE, "..", "kmerjs_amd", "csrc")
    subprocess.run([HIPCC, "-O2", "-std=c++17", "-I", inc, "-o", str(exe), src], check=True,
                   capture_output=True, timeout=300)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert " 0 of " in r.stdout
