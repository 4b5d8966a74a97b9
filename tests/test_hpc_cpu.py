"""`--hpc` without a GPU: the plain-Python statement (tests/hpc_cases.py) on
hand-written cases, the option combinations that are refused before any
device work, the help texts and the header."""

from __future__ import annotations

import os

import numpy as np
import pytest
from click.testing import CliRunner

import hpc_cases as hc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
A, C, G, T, N_, F = 0, 1, 2, 3, 4, 8  # codes; F: a record's first character


def test_codes_statement_by_hand():
    #        A      A  A  C  C  N   N   A  | A      A  G  | (empty) | T
    codes = [A | F, A, A, C, C, N_, N_, A, A | F, A, G, T | F]
    out, rec, orig = hc.hpc_codes(codes, [0, 8, 11, 11])
    assert out.tolist() == [A | F, C, N_, N_, A, A | F, G, T | F]
    assert orig.tolist() == [0, 3, 5, 6, 7, 8, 10, 11]
    assert rec.tolist() == [0, 5, 7, 7]  # the empty record stays empty
    # a masked base (bit 2 on a base code) separates its neighbours and is kept
    out, _, orig = hc.hpc_codes([A | F, A | 4, A, A], [0])
    assert out.tolist() == [A | F, A | 4, A] and orig.tolist() == [0, 1, 2]
    # bases before rec_seq[0] follow the same rule; entries past n are clamped
    out, rec, _ = hc.hpc_codes([G, G, G, C | F, C], [3, 99])
    assert out.tolist() == [G, C | F] and rec.tolist() == [1, 2]
    out, rec, orig = hc.hpc_codes([], [0, 0])
    assert len(out) == 0 and rec.tolist() == [0, 0] and len(orig) == 0


def test_text_statement_by_hand():
    fa = b">r1 desc\nAAAC\nCCGg\n>empty\n>r3\nNNNaATT\n"
    assert hc.hpc_text(fa) == b">r1 desc\nACG\n>empty\n>r3\nNNNaT\n"
    fq = b"@q1 x\nAACCGGTT\n+\nIIIIIIII\n@q2\nACGT\n+\nIIII\n"
    assert hc.hpc_text(fq) == b">q1 x\nACGT\n>q2\nACGT\n"
    assert hc.hpc_seq("AAACCG") == ("ACG", [0, 3, 5])


def test_map_span_by_hand():
    seq = "AAACCGGGGT"  # compressed ACGT, columns 0 3 5 9
    comp, cols = hc.hpc_seq(seq)
    assert comp == "ACGT" and cols == [0, 3, 5, 9]
    assert hc.map_span(0, 0, cols, len(seq)) == (0, 0)
    assert hc.map_span(1, 3, cols, len(seq)) == (3, 9)   # C and G with their whole runs
    assert hc.map_span(0, 4, cols, len(seq)) == (0, 10)  # to the record's last base
    assert hc.map_span(2, 3, cols, len(seq)) == (5, 9)   # the stretch ends inside the original's run of G
    seq2 = "ACGTT"
    assert hc.map_span(1, 4, hc.hpc_seq(seq2)[1], len(seq2)) == (1, 5)  # the last base's run reaches the end


def test_vary_homopolymers_keeps_the_compressed_sequence():
    rng = np.random.default_rng(3)
    seq = "".join("ACGT"[i] for i in rng.integers(0, 4, 2000))
    var = hc.vary_homopolymers(seq, rng)
    assert var != seq and hc.hpc_seq(var)[0] == hc.hpc_seq(seq)[0]


# ------------------------------------------------------------------------ CLI


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp("hpc_cpu")
    (d / "a.fa").write_bytes(b">a\nAACCGGTTAACCGGTT\n")
    (d / "r.fq").write_bytes(b"@r/1\nAACCGGTTAACC\n+\nIIIIIIIIIIII\n@r/2\nAACCGGTTAACC\n+\nIIIIIIIIIIII\n")
    return d


def _refused(argv, needle):
    from kman_amd.scripts.kmer import main

    r = CliRunner().invoke(main, [str(a) for a in argv])
    assert r.exit_code != 0
    assert isinstance(r.exception, AssertionError), r.output
    assert needle in str(r.exception), str(r.exception)
    assert "\n" not in str(r.exception)  # a one-line reason


def test_screen_refusals(files):
    d = files
    _refused(["screen", d / "r.fq", d / "a.fa", d / "o.tsv", 5, "--hpc", "--solid", 1, "--correct"],
             "--hpc with --correct")
    _refused(["screen", d / "r.fq", d / "a.fa", d / "o.tsv", 5, "--hpc", "--solid", 1, "--mate", d / "r.fq"],
             "--hpc with --solid")
    _refused(["screen", d / "r.fq", d / "a.fa", d / "o.tsv", 5, "--hpc", "--solid", 1, "--interleaved"],
             "--hpc with --solid")
    assert not (d / "o.tsv").exists()


def test_count_refusals_follow_canonical(files):
    d = files
    _refused(["count", d / "a.fa", d / "o.txt", 5, "--hpc", "-r"], "--hpc with -r")
    _refused(["count", d / "a.fa", d / "o.txt", 5, "--hpc", "-B", d], "--hpc with -B")
    _refused(["count", d / "a.fa", d / "o.txt", 5, "--hpc", "-m", "VEC_COUNT"], "--hpc needs -m SEQ_COUNT")
    # the same three with --canonical are refused today
    _refused(["count", d / "a.fa", d / "o.txt", 5, "--canonical", "-r"], "--canonical with -r")
    _refused(["count", d / "a.fa", d / "o.txt", 5, "--canonical", "-B", d], "--canonical with -B")
    _refused(["count", d / "a.fa", d / "o.txt", 5, "--canonical", "-m", "VEC_COUNT"], "need -m SEQ_COUNT")
    assert not (d / "o.txt").exists()


def test_multi_gpu_route_follows_canonical(monkeypatch):
    from kman_amd import launch
    from kman_amd.scripts import kmer

    monkeypatch.setattr(launch, "distributed", lambda: True)
    monkeypatch.setattr(launch, "log_solo", lambda what: None)
    for solo, want in ((True, False), (False, None)):
        monkeypatch.setattr(launch, "solo_rank", lambda solo=solo: solo)
        assert kmer._multi_gpu(21, None, "SEQ_COUNT", None, "fasta", canonical=True) is want
        assert kmer._multi_gpu(21, None, "SEQ_COUNT", None, "fasta", hpc=True) is want
    assert kmer._multi_gpu(21, None, "SEQ_COUNT", None, "fasta") is True


@pytest.mark.parametrize("cmd", ["count", "hist", "sets", "screen", "classify"])
def test_help_names_the_flag(cmd):
    from kman_amd.scripts.kmer import main

    r = CliRunner().invoke(main, [cmd, "--help"])
    assert r.exit_code == 0 and "--hpc" in r.output


@pytest.mark.parametrize("cmd", ["uniq", "batch"])
def test_position_commands_do_not_take_the_flag(cmd):
    from kman_amd.scripts.kmer import main

    r = CliRunner().invoke(main, [cmd, "--help"])
    assert r.exit_code == 0 and "--hpc" not in r.output


def test_header_and_binding_declare_the_kernel():
    from kman_amd import _native as N

    with open(os.path.join(ROOT, "include", "kman.h")) as fh:
        header = fh.read()
    assert "int kman_hpc_records(kman_ctx *ctx, const uint8_t *d_codes, uint64_t n_bases," in header
    assert "#define KMAN_HPC_TILE %d" % N.KMAN_HPC_TILE in header
    assert "#define KMAN_ABI_VERSION 1" in header
