"""bench.py's plain single-GPU run on a small input: the result line of a run
without --full (steps as asked, ms_per_step, no line that takes a run of its
own) and the rows `--dump-outputs` writes, bit-exact against the numpy oracle
of the same synthetic FASTA."""

from __future__ import annotations

import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu

BASES, K = 3_000_000, 21  # ~3 M rows, more than the 2^20 that are sampled: the block sample is exercised


@pytest.fixture(scope="module")
def oracle_rows():
    """(n_kmers, keys, pos) of `kmer uniq` on the benchmark's input at BASES bases."""
    import inputs
    import np_oracle

    records = np_oracle.parse_fasta(inputs.syn_numpy(BASES, 1))
    keys, pos = np_oracle.stream_kmers(records, K)
    uk, up = np_oracle.rle_uniq(*np_oracle.stable_sort(keys, pos))
    return len(keys), uk, up


def _run(tmp_path, name, *extra):
    d = tmp_path / name
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--bases", str(BASES), "--k", str(K), "--dump-outputs", str(d)] + list(extra),
                       capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0]), {n[:-4]: np.load(d / n) for n in sorted(os.listdir(d))}


def test_plain_run_line_and_dumped_rows(tmp_path, oracle_rows):
    n_kmers, uk, up = oracle_rows
    out, dump = _run(tmp_path, "a")
    assert out["steps"] == 3 and out["warmup"] == 1 and out["n_gpus"] == 1 and out["unit"] == "k-mers/s"
    assert out["higher_is_better"] is True and out["dtype"] == "u64" and out["ms_per_step"] > 0
    assert abs(out["value"] - n_kmers / (out["ms_per_step"] / 1e3)) <= 1e-6 * out["value"]
    assert out["config"]["kmers_per_step_per_gpu"] == n_kmers
    # nothing that takes a run of its own
    assert out["cpu_baseline"] is None
    assert not {"output", "pinned_host", "file_to_file", "file_to_file_config2"} & set(out)

    assert sorted(dump) == ["counts", "keys", "rows", "vals"]
    assert all(a.dtype == np.float64 for a in dump.values())
    assert sum(a.nbytes for a in dump.values()) <= 64 << 20
    assert list(dump["counts"]) == [n_kmers, len(uk)]
    rows = dump["rows"].astype(np.int64)
    assert len(rows) == 1 << 20 and rows[0] == 0 and rows[-1] == len(uk) - 1
    keys = (dump["keys"][:, 0].astype(np.uint64) << np.uint64(32)) | dump["keys"][:, 1].astype(np.uint64)
    np.testing.assert_array_equal(keys, uk[rows])
    np.testing.assert_array_equal(dump["vals"].astype(np.uint64), up[rows])

    # the same arguments again: the same rows, value for value
    _, again = _run(tmp_path, "b")
    for name, a in dump.items():
        np.testing.assert_array_equal(a, again[name])
