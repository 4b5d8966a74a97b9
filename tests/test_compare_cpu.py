"""`kmer compare` without a GPU: the plain-Python statement
(tests/compare_cases.py) pinned to hand-written numbers, the metrics' edge
cases, engine.compare_rows and the host formatters against the statement,
the ABI's constants and signature, and every refusal of the command, raised
before any device work or output file."""

from __future__ import annotations

import math
import os
import re

import numpy as np
import pytest
from click.testing import CliRunner

import compare_cases as cmp


def test_helper_on_a_hand_worked_example():
    """Three inputs over six k-mers, k = 4:
         AAAA  a b c      CCCC  a b        GGGG  b c
         ACGT  a          TTTT  a          AACC  c      (and ACGT twice in a)"""
    a = [("a", "AAAANCCCCNACGTNTTTT"), ("a2", "ACGT")]
    b = [("b", "AAAANCCCCNGGGG")]
    c = [("c", "AAAANGGGGNAACC")]
    G, occ, private = cmp.compare([a, b, c], 4)
    assert G == [[4, 2, 1], [2, 3, 2], [1, 2, 3]]
    assert occ == [0, 3, 2, 1] and private == [2, 0, 1]
    # -L 2: only ACGT of a is left
    assert cmp.compare([a, b, c], 4, min_count=2) == ([[1, 0, 0], [0, 0, 0], [0, 0, 0]], [0, 1, 0, 0], [1, 0, 0])
    # canonical: TTTT folds into AAAA, GGGG into CCCC
    G, occ, private = cmp.compare([a, b, c], 4, canonical=True)
    assert G == [[3, 2, 2], [2, 2, 2], [2, 2, 3]] and occ == [0, 2, 0, 2] and private == [1, 0, 1]
    # masks directly: bits at or above n_colors are cut; a row of none of the colours is occ[0]
    masks = [0b111, 0b011, 0b110, 0b001, 0b001, 0b100, 0b1000, 0]
    assert cmp.mask_gram(masks, 3) == ([[4, 2, 1], [2, 3, 2], [1, 2, 3]], [2, 3, 2, 1], [2, 0, 1])
    assert cmp.mask_gram(masks, 1) == ([[4]], [4, 4], [4])
    assert cmp.mask_gram([], 2) == ([[0, 0], [0, 0]], [0, 0, 0], [0, 0])
    top = (1 << 64) - 1
    G, occ, private = cmp.mask_gram([top, top, 1 << 63], 64)
    assert G[63][63] == 3 and G[0][63] == 2 and occ[64] == 2 and occ[1] == 1 and private[63] == 1
    # the rows and the files of the first example
    G = [[4, 2, 1], [2, 3, 2], [1, 2, 3]]
    r = cmp.rows(G, 4)
    assert [x[:5] for x in r] == [(0, 1, 4, 3, 2), (0, 2, 4, 3, 1), (1, 2, 3, 3, 2)]
    assert r[0][5:8] == (2 / 5, 2 / 4, 2 / 3)
    assert r[0][8] == pytest.approx(-math.log(2 * 0.4 / 1.4) / 4)
    assert cmp.lines(["a", "b", "c"], G, 4) == (b"a\tb\t4\t3\t2\t0.400000\t0.500000\t0.666667\t0.139904\n"
                                                 b"a\tc\t4\t3\t1\t0.166667\t0.250000\t0.333333\t0.313191\n"
                                                 b"b\tc\t3\t3\t2\t0.500000\t0.666667\t0.666667\t0.101366\n")
    assert cmp.matrix(["a", "b", "c"], G, 4, "shared") == b"3\na\t4\t2\t1\nb\t2\t3\t2\nc\t1\t2\t3\n"
    assert cmp.matrix(["a", "b", "c"], G, 4, "containment") == (b"3\na\t1.000000\t0.500000\t0.250000\n"
                                                                b"b\t0.666667\t1.000000\t0.666667\n"
                                                                b"c\t0.333333\t0.666667\t1.000000\n")
    assert cmp.matrix(["a", "b", "c"], G, 4).startswith(b"3\na\t0.000000\t0.139904\t0.313191\nb\t0.139904\t0.000000")
    assert cmp.matrix(["a", "b", "c"], G, 4, "jaccard").splitlines()[1] == b"a\t1.000000\t0.400000\t0.166667"
    assert cmp.occupancy([0, 3, 2, 1]) == b"1\t3\n2\t2\n3\t1\n"
    assert cmp.summary(["a", "b", "c"], G, [2, 0, 1]) == b"a\t4\t2\nb\t3\t0\nc\t3\t1\n"


def test_metric_edge_cases():
    from kman_amd import engine

    for fn in (cmp.metrics, engine.compare_metrics):
        assert fn(0, 0, 0, 21) == (0.0, 0.0, 0.0, 1.0)  # two empty inputs
        assert fn(0, 7, 0, 21) == (0.0, 0.0, 0.0, 1.0)  # one empty input
        assert fn(7, 7, 7, 21) == (1.0, 1.0, 1.0, 0.0)  # identical inputs: D is exactly 0
        assert fn(5, 9, 0, 21) == (0.0, 0.0, 0.0, 1.0)  # disjoint inputs
        assert fn(4, 8, 4, 3) == (0.5, 1.0, 0.5, -math.log(2 * 0.5 / 1.5) / 3)  # one input inside the other
        j, ca, cb, d = fn(10 ** 6, 10 ** 6, 1, 1)  # a tiny J at k = 1: clamped to 1
        assert d == 1.0 and 0 < j < 1e-6
        big = 1 << 62  # counts past 2^53
        assert fn(big, big, big, 32) == (1.0, 1.0, 1.0, 0.0)
    # a matrix with an empty input: its diagonal is 0 (jaccard, containment) and 0 (dist)
    G = [[3, 0], [0, 0]]
    assert cmp.matrix(["x", "e"], G, 5, "jaccard") == b"2\nx\t1.000000\t0.000000\ne\t0.000000\t0.000000\n"
    assert cmp.matrix(["x", "e"], G, 5, "containment") == b"2\nx\t1.000000\t0.000000\ne\t0.000000\t0.000000\n"
    assert cmp.matrix(["x", "e"], G, 5, "dist") == b"2\nx\t0.000000\t1.000000\ne\t1.000000\t0.000000\n"


def test_engine_rows_and_formatters_agree_with_the_statement():
    from kman_amd import engine

    for nc, k in ((2, 5), (3, 21), (7, 32), (64, 11)):
        masks = cmp.mask_cases(200, nc, seed=nc)["sparse" if nc == 64 else "dense"]
        masks[::9] = 0
        G, occ, private = cmp.mask_gram(masks, nc)
        if nc == 7:
            G[3] = [0] * nc  # an empty input
            for row in G:
                row[3] = 0
        labels = ["in%d" % c for c in range(nc)]
        g = np.asarray(G, dtype=np.uint64)
        assert engine.compare_rows(g, k) == cmp.rows(G, k)
        assert engine.emit_compare(labels, g, k) == cmp.lines(labels, G, k)
        for metric in cmp.METRICS:
            assert engine.emit_compare_matrix(labels, g, k, metric) == cmp.matrix(labels, G, k, metric)
        assert engine.emit_compare_matrix(labels, g, k) == cmp.matrix(labels, G, k, "dist")
        assert engine.emit_occupancy(np.asarray(occ, dtype=np.uint64)) == cmp.occupancy(occ)
        assert engine.emit_compare_summary(labels, g, np.asarray(private, dtype=np.uint64)) == \
            cmp.summary(labels, G, private)
    with pytest.raises(AssertionError):
        engine.emit_compare_matrix(["a", "b"], np.zeros((2, 2), np.uint64), 5, "bray-curtis")
    with pytest.raises(AssertionError):
        engine.emit_compare(["a"], np.zeros((2, 2), np.uint64), 5)
    with pytest.raises(AssertionError):
        engine.compare_rows(np.zeros((2, 3), np.uint64), 5)


def test_header_signature_and_constants_agree():
    from kman_amd import _native as N

    with open(os.path.join(os.path.dirname(N.HERE), "include", "kman.h")) as fh:
        text = fh.read()
    for name in ("KMAN_GRAM_THREADS", "KMAN_GRAM_MAX_BLOCKS"):
        m = re.search(r"#define\s+%s\s+(\d+)\s" % name, text)
        assert m and int(m.group(1)) == getattr(N, name), name
    m = re.search(r"#define\s+KMAN_GRAM_MAX_ROWS\s+\(1ull << (\d+)\)", text)
    assert m and 1 << int(m.group(1)) == N.KMAN_GRAM_MAX_ROWS
    # the 32-bit accumulators of a block: 64 per step and wave, four waves
    steps = N.KMAN_GRAM_MAX_ROWS // (N.KMAN_GRAM_MAX_BLOCKS * N.KMAN_GRAM_THREADS)
    assert 64 * (N.KMAN_GRAM_THREADS // 64) * steps < 1 << 32
    assert "kman_mask_gram" in N.header_symbols() and len(N.SIGNATURES["kman_mask_gram"][1]) == 7
    decl = re.search(r"\bint kman_mask_gram\(([^;]*)\);", text)
    assert decl and len(decl.group(1).split(",")) == 7
    assert sorted(N.SIGNATURES) == N.header_symbols()
    with open(os.path.join(N.HERE, "csrc", "Makefile")) as fh:
        assert "gram.hip" in fh.read()
    with open(os.path.join(N.HERE, "csrc", "gram.hip")) as fh:
        src = fh.read()
    assert "__ballot" in src and '"gram"' in src and "asm" not in src


# -------------------------------------------------------------------- the CLI


@pytest.fixture()
def inputs(tmp_path):
    a = tmp_path / "a.fa"
    a.write_bytes(b">s\nTTGCAACGTACG\n")
    b = tmp_path / "b.fa"
    b.write_bytes(b">t\nGGGGGGCCCCACGT\n")
    fq = tmp_path / "reads.fq"
    fq.write_bytes(b"@q\nACGTACGTTG\n+\nIIIIIIIIII\n")
    return a, b, fq


def test_help_shows_every_option():
    from kman_amd.scripts.kmer import main

    run = CliRunner()
    text = run.invoke(main, ["compare", "--help"]).output
    for opt in ("OUTPUT", " K", "INPUT INPUT [INPUT ...]", "--canonical", "-f,", "--format", "-q,", "--min-qual",
                "--phred-offset", "-L,", "--min-count", "-U,", "--max-count", "--hpc", "--matrix", "--metric",
                "--occupancy", "--summary", "Not part of the reference", "Bray-Curtis", "sketching"):
        assert opt in text, opt
    assert "READS" not in text and "--specific" not in text
    assert "compare" in run.invoke(main, ["--help"]).output


def _refused_cases(tmp_path, inputs):
    """name -> (argv, the message)."""
    a, b, fq = inputs
    out = tmp_path / "out.tsv"
    d = tmp_path / "d"
    d.mkdir()
    (d / "a.fasta").write_bytes(b">u\nACGTACGT\n")
    many = []
    for i in range(65):
        path = d / ("m%d.fa" % i)
        path.write_bytes(b">u\nACGTACGT\n")
        many.append(str(path))
    (d / "with\ttab.fa").write_bytes(b">u\nACGTACGT\n")
    sa, sb = str(a), str(b)
    return {
        "no_input": ([str(out), "5"], "2 to 64 INPUT"),
        "one_input": ([str(out), "5", sa], "2 to 64 INPUT"),
        "65_inputs": ([str(out), "5"] + many, "2 to 64 INPUT"),
        "k_1": ([str(out), "1", sa, sb], "k must be >= 1"),
        "k_33": ([str(out), "33", sa, sb], "K <= 32"),
        "equal_labels": ([str(out), "5", sa, str(d / "a.fasta")], "label 'a'"),
        "same_input_twice": ([str(out), "5", sa, sb, sa], "label 'a'"),
        "label_tab": ([str(out), "5", sa, str(d / "with\ttab.fa")], "tab"),
        "metric_without_matrix": ([str(out), "5", sa, sb, "--metric", "jaccard"], "--metric needs --matrix"),
        "output_is_input": ([sb, "5", sa, sb], "same file"),
        "matrix_is_input": ([str(out), "5", sa, sb, "--matrix", sa], "same file"),
        "matrix_is_output": ([str(out), "5", sa, sb, "--matrix", str(out)], "same file"),
        "summary_is_occupancy": ([str(out), "5", sa, sb, "--summary", str(d / "x"), "--occupancy", str(d / "x")],
                                 "same file"),
        "min_qual_without_fastq": ([str(out), "5", "-q", "20", sa, sb], "--min-qual"),
        "min_above_max": ([str(out), "5", "-L", "6", "-U", "5", sa, sb], "--min-count 6 is greater than --max-count 5"),
    }


REFUSED = ["no_input", "one_input", "65_inputs", "k_1", "k_33", "equal_labels", "same_input_twice", "label_tab",
           "metric_without_matrix", "output_is_input", "matrix_is_input", "matrix_is_output", "summary_is_occupancy",
           "min_qual_without_fastq", "min_above_max"]


@pytest.mark.parametrize("case", REFUSED)
def test_refused_before_any_device_work_or_output(case, inputs, tmp_path, monkeypatch):
    from kman_amd import _native, engine
    from kman_amd.scripts.kmer import main

    def no_device(*a, **kw):
        raise RuntimeError("device work before the options were checked")

    monkeypatch.setattr(engine, "default_device", no_device)
    monkeypatch.setattr(engine, "Device", no_device)
    monkeypatch.setattr(_native, "lib", no_device)
    cases = _refused_cases(tmp_path, inputs)
    assert sorted(cases) == sorted(REFUSED)
    before = {p: p.read_bytes() for p in tmp_path.rglob("*") if p.is_file()}
    argv, msg = cases[case]
    r = CliRunner().invoke(main, ["compare"] + argv)
    assert isinstance(r.exception, AssertionError), (r.exception, r.output)
    assert msg in str(r.exception)
    assert {p: p.read_bytes() for p in tmp_path.rglob("*") if p.is_file()} == before  # nothing made or overwritten


@pytest.mark.parametrize("argv", [["5", "-L", "0"], ["5", "--metric", "bray-curtis"], ["5", "-q", "94"],
                                  ["five"], ["5", "--specific"]])
def test_usage_errors(argv, inputs, tmp_path):
    from kman_amd.scripts.kmer import main

    out = tmp_path / "out.tsv"
    r = CliRunner().invoke(main, ["compare", str(out)] + argv + [str(inputs[0]), str(inputs[1])])
    assert r.exit_code == 2 and not out.exists()
    r = CliRunner().invoke(main, ["compare", str(out), "5", str(inputs[0]), "no/such/file.fa"])
    assert r.exit_code == 2 and not out.exists()


def test_min_qual_is_taken_when_one_input_is_fastq(inputs, tmp_path, monkeypatch):
    from kman_amd import engine
    from kman_amd.scripts.kmer import main

    class Reached(Exception):
        pass

    def device(*a, **kw):
        raise Reached()

    monkeypatch.setattr(engine, "default_device", device)
    for v in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "KMAN_DIST"):
        monkeypatch.delenv(v, raising=False)
    out = tmp_path / "out.tsv"
    a, b, fq = inputs
    for argv in ([str(fq), str(a)], [str(a), str(b), str(fq)]):
        r = CliRunner().invoke(main, ["compare", str(out), "5", "-q", "20"] + argv)
        assert isinstance(r.exception, Reached), (r.exception, r.output)
    assert not out.exists()


def test_runs_on_rank_0_alone(inputs, tmp_path, monkeypatch):
    from kman_amd import engine
    from kman_amd.scripts.kmer import main

    def no_device(*a, **kw):
        raise RuntimeError("a rank other than 0 asked for the device")

    monkeypatch.setattr(engine, "default_device", no_device)
    monkeypatch.setenv("WORLD_SIZE", "4")
    monkeypatch.setenv("RANK", "2")
    monkeypatch.setenv("LOCAL_RANK", "2")
    monkeypatch.delenv("KMAN_DIST", raising=False)
    out = tmp_path / "out.tsv"
    r = CliRunner().invoke(main, ["compare", str(out), "5", str(inputs[0]), str(inputs[1])])
    assert r.exception is None and r.exit_code == 0 and not out.exists()
    r = CliRunner().invoke(main, ["compare", str(out), "40", str(inputs[0]), str(inputs[1])])
    assert isinstance(r.exception, AssertionError)  # (refused on every rank)
