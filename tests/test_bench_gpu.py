"""bench.py on the device: a plain run prints the headline line and nothing
that needs runs of its own; --dump-outputs writes the last timed step's result
(checked against the oracle); --full adds the other legs."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests.conftest import REPO

pytestmark = pytest.mark.gpu

BENCH = os.path.join(REPO, "bench.py")
READS = 20000
FULL_ONLY = ("distinct_kmers", "accepted_windows", "roofline", "scan_kernel_ms", "pipelined", "cpu_baseline",
             "end_to_end", "template_matching", "pcie_inclusive_ms")


def run_bench(*argv):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    p = subprocess.run([sys.executable, BENCH, "--gpus", "1"] + list(argv), env=env, capture_output=True, text=True,
                       timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [x for x in p.stdout.splitlines() if x.startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:]
    return json.loads(lines[0])


@pytest.fixture(scope="module")
def plain(tmp_path_factory):
    d = tmp_path_factory.mktemp("dump")
    line = run_bench("--steps", "2", "--warmup", "1", "--reads", str(READS), "--dump-outputs", str(d))
    return line, {f[:-4]: np.load(os.path.join(d, f)) for f in os.listdir(d)}


def test_plain_line_is_the_headline(plain):
    line, _ = plain
    assert line["unit"] == "k-mers/s" and line["higher_is_better"] is True and line["dtype"] == "u8"
    assert line["steps"] == 2 and line["warmup"] == 1 and line["n_gpus"] == 1
    assert line["ms_per_step"] > 0
    # value = windows of a step / time of a step
    windows = READS * 2 * (150 - 16 + 1)
    assert line["config"]["windows_per_step"] == windows
    assert line["value"] == pytest.approx(windows / (line["ms_per_step"] * 1e-3), rel=1e-9)
    assert not [x for x in FULL_ONLY if x in line]


def test_dump_outputs_equal_the_oracle(plain):
    from oracle import oracle
    _, arrays = plain
    assert all(a.dtype in (np.float32, np.float64) for a in arrays.values())
    want = oracle.count_buffer(oracle.synth_fastq(1, 0, READS), b"ATGAC", 16, 1)
    n, dev_sum, n_rec, rec_sum = (int(x) for x in arrays["totals"])
    assert (n_rec, rec_sum) == (0, 0)                       # (synthetic reads are A/C/G/T only)
    assert sorted(arrays) == ["counts", "firsts", "keys", "rows", "totals"]     # (no empty record arrays)
    assert all(a.size for a in arrays.values())
    assert n == len(want) and dev_sum == sum(c for _, c in want)
    assert arrays["rows"].tolist() == list(range(n))        # (small result: every entry dumped)
    keys = arrays["keys"]
    assert keys.shape == (n, 16)
    got = [bytes(r) for r in keys.astype(np.uint8)]
    assert got == [key for key, _ in want]
    assert arrays["counts"].tolist() == [float(c) for _, c in want]
    assert bool((np.diff(arrays["firsts"]) > 0).all())      # Map (first-occurrence) order


def test_full_table_mode_line_and_dump(tmp_path):
    """--full (side legs off) on a small C3-style table-mode run: the extra
    fields are there, and the dumped table statistics are those of the
    oracle's Map."""
    from oracle import oracle
    n = 1000
    line = run_bench("--full", "--config", "c3", "--reads", str(n), "--steps", "1", "--warmup", "1",
                     "--no-cpu-baseline", "--no-pcie", "--no-e2e", "--no-match", "--no-pipelined",
                     "--dump-outputs", str(tmp_path))
    assert line["ms_per_step"] > 0 and line["roofline"]["kernel_ms"] > 0 and "table_phase_ms" in line
    want = oracle.count_buffer(oracle.synth_fastq(3, 0, n), b"", 31, 1)
    comp = bytes.maketrans(b"ACGT", b"TGCA")
    canonical = {min(key, key.translate(comp)[::-1]) for key, _ in want}
    assert os.listdir(tmp_path) == ["table.npy"]
    t = np.load(tmp_path / "table.npy")
    assert t.dtype == np.float64 and t.shape == (5,)
    assert int(t[0]) == len(canonical) == line["canonical_kmers"]
    assert int(t[1]) == len(want) == line["distinct_kmers"]
    assert int(t[2]) == sum(c for _, c in want) == n * 2 * (150 - 31 + 1) == line["accepted_windows"]
    assert 0 <= t[3] < 2 ** 32 and 0 <= t[4] < 2 ** 32
