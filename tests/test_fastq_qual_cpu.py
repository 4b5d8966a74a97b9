"""FASTQ quality threshold on the CPU: the restatement's known answers, the
``--min-qual`` / ``--phred-offset`` options of every command, the ABI entry
and the host-side validation that runs before any device work."""

from __future__ import annotations

import os

import pytest

import fastq_cases as fq
from fastq_qual_cases import mask_fastq


def test_mask_fastq_known_answers():
    # '5' is Q20 at offset 33: '4' (Q19) is below, '5' is not
    assert mask_fastq(b"@a x\nACGT\n+\n4554\n", 20) == (b">a x\nNCGN\n", 2)
    # min_qual 0 is off, whatever the bytes
    assert mask_fastq(b"@a\nACGT\n+\n!\x01!!\n", 0) == (b">a\nACGT\n", 0)
    # a blank inside the sequence line: columns, not code indices, pair the bytes;
    # the blank itself and the trailing blank are not kept bytes
    assert mask_fastq(b"@a\nA C \n+\nI!!!\n", 20) == (b">a\nA N \n", 1)
    # (a tab with a base after it is a kept byte: its code is already that of an N)
    assert mask_fastq(b"@a\nAC GT\tA \n+\n!IIII!!!\n", 20) == (b">a\nNC GTNN \n", 3)
    assert mask_fastq(b"@b\nAC\t\n+\n!!!\n", 20) == (b">b\nNN\t\n", 2)  # (a trailing tab is not)
    # CRLF and a lone CR
    assert mask_fastq(b"@a\r\nACGT\r\n+\r\nI!I!\r\n", 20) == (b">a\nANGN\n", 2)
    assert mask_fastq(b"@a\rAC\r+\r!I\r", 20) == (b">a\nNC\n", 1)
    # a zero-length read between two others, and one cut after its '+'
    assert mask_fastq(b"@a\nAC\n+\n!!\n@r\n\n+\n\n@b\nG\n+\n!\n", 1) == (b">a\nNN\n>r\n\n>b\nN\n", 3)
    assert mask_fastq(b"@a\nAC\n+\nI!\n@r\n\n+", 20) == (b">a\nAN\n>r\n\n", 1)
    # offset 64: 'h' is Q40, 'I' would be negative
    assert mask_fastq(b"@a\nACGT\n+\nhIJK\n", 10, 64) == (b">a\nANGT\n", 1)
    assert mask_fastq(b"@a\nACGT\n+\nhIJK\n", 10, 33) == (b">a\nACGT\n", 0)
    # everything and nothing: T = '~' masks all but '~'; T = '"' masks only '!'
    assert mask_fastq(b"@a\nACGTN\n+\n!I}~}\n", 93) == (b">a\nNNNTN\n", 4)
    assert mask_fastq(b"@a\nACGTN\n+\n\"I}~}\n", 1) == (b">a\nACGTN\n", 0)
    # an N already there still counts; lower case is masked to 'N'
    assert mask_fastq(b"@a\nNacg\n+\n!!II\n", 20) == (b">a\nNNcg\n", 2)
    # quality bytes >= 0x80 compare unsigned
    assert mask_fastq(b"@a\nAC\n+\n\xff!\n", 93) == (b">a\nAN\n", 1)


def test_mask_fastq_errors_propagate():
    with pytest.raises(AssertionError, match="FASTQ record 1: quality length 7 != sequence length 8"):
        mask_fastq(b"@a\nACGTACGT\n+\nIIIIIII\n", 20)
    with pytest.raises(AssertionError, match="premature end of file or empty file"):
        mask_fastq(b"", 20)


def test_mask_fastq_keeps_the_records():
    import np_oracle

    text = fq.mixed_reads()
    plain = np_oracle.parse_fasta(fq.fastq_to_fasta(text))
    for q, off in ((1, 33), (20, 33), (93, 33), (10, 64)):
        fasta, n = mask_fastq(text, q, off)
        recs = np_oracle.parse_fasta(fasta)
        assert [t for t, _ in recs] == [t for t, _ in plain]
        assert [len(s) for _, s in recs] == [len(s) for _, s in plain]
        changed = sum(a != b for (_, x), (_, y) in zip(recs, plain) for a, b in zip(x, y))
        assert 0 < changed <= n  # (an N that is masked does not change)
    assert mask_fastq(text, 0)[0] == fq.fastq_to_fasta(text)


@pytest.mark.parametrize("cmd", ["count", "uniq", "batch", "hist"])
def test_commands_take_quality_options(cmd, tmp_path):
    from click.testing import CliRunner

    from kman_amd.scripts.kmer import main

    run = CliRunner()
    r = run.invoke(main, [cmd, "--help"])
    assert r.exit_code == 0
    for word in ("--min-qual", "-q", "--phred-offset"):
        assert word in r.output
    src, out = tmp_path / "in.fq", tmp_path / "out"
    src.write_bytes(b"@r\nACGT\n+\nIIII\n")
    for bad in (["-q", "94"], ["-q", "-1"], ["--min-qual", "94"], ["--phred-offset", "50"]):
        r = run.invoke(main, [cmd, str(src), str(out), "3"] + bad)
        assert r.exit_code == 2 and not out.exists(), bad
    # good values pass the option parser: the command then stops at k = 1
    for good in (["-q", "0"], ["-q", "93"], ["-q", "20", "--phred-offset", "64"], ["--phred-offset", "33"]):
        r = run.invoke(main, [cmd, str(src), str(out), "1"] + good)
        assert r.exit_code != 2, good


@pytest.mark.parametrize("cmd", ["count", "uniq", "batch", "hist"])
def test_min_qual_needs_fastq_input(cmd, tmp_path):
    from kman_amd.scripts.kmer import main

    fa, fqp, out = tmp_path / "in.fa", tmp_path / "in.fq", tmp_path / "out"
    fa.write_bytes(b">r\nACGTACGT\n")
    fqp.write_bytes(b"@r\nACGTACGT\n+\nIIIIIIII\n")
    for argv in ([cmd, str(fa), str(out), "3", "-q", "20"],
                 [cmd, str(fqp), str(out), "3", "-q", "20", "-f", "fasta"],
                 [cmd, str(fa), str(out), "3", "--min-qual", "1", "--phred-offset", "64"]):
        with pytest.raises(AssertionError, match="--min-qual needs fastq input"):
            main(argv, standalone_mode=False)
        assert not out.exists()


@pytest.mark.parametrize("cmd", ["count", "uniq"])
def test_min_qual_refuses_previous_batches(cmd, tmp_path):
    from kman_amd.scripts.kmer import main

    fqp, out, prev = tmp_path / "in.fq", tmp_path / "out", tmp_path / "prev"
    fqp.write_bytes(b"@r\nACGTACGT\n+\nIIIIIIII\n")
    prev.mkdir()
    with pytest.raises(AssertionError, match="--min-qual needs fastq input"):
        main([cmd, str(fqp), str(out), "3", "-q", "20", "-B", str(prev)], standalone_mode=False)
    assert not out.exists()


def test_native_signature_and_header():
    from ctypes import POINTER, c_uint32, c_uint64

    from conftest import ROOT
    from kman_amd import _native

    res, argt = _native.SIGNATURES["kman_parse_fastq_q"]
    res0, argt0 = _native.SIGNATURES["kman_parse_fastq"]
    assert res == res0 and argt[:len(argt0)] == argt0 and argt[len(argt0):] == [c_uint32, POINTER(c_uint64)]
    with open(os.path.join(ROOT, "include", "kman.h")) as fh:
        assert "int kman_parse_fastq_q(kman_ctx *ctx" in fh.read()
    assert "kman_parse_fastq_q" in _native.header_symbols()


class _NoDevice:
    """Stands for a Device: any use of it fails the test."""

    def __getattr__(self, name):
        raise RuntimeError("device touched (%s) before the options were checked" % name)


@pytest.mark.parametrize("kw, msg", [
    (dict(min_qual=94), "min_qual"),
    (dict(min_qual=-1), "min_qual"),
    (dict(min_qual=2.5), "min_qual"),
    (dict(min_qual="20"), "min_qual"),
    (dict(min_qual=True), "min_qual"),
    (dict(min_qual=20, phred_offset=50), "phred_offset"),
    (dict(min_qual=0, phred_offset=0), "phred_offset"),
])
def test_engine_rejects_bad_options_before_the_device(kw, msg):
    from kman_amd import engine
    from kman_amd.batcher import FastaBatcher

    text = b"@r\nACGT\n+\nIIII\n"
    with pytest.raises(AssertionError, match=msg):
        engine.parse_fastq(_NoDevice(), text, **kw)
    with pytest.raises(AssertionError, match=msg):
        engine.parse(_NoDevice(), text, "fastq", **kw)
    with pytest.raises(AssertionError, match=msg):
        engine.parse_file(_NoDevice(), "no such file", "fastq", **kw)
    with pytest.raises(AssertionError, match=msg):
        FastaBatcher(fmt="fastq", **kw)


def test_engine_min_qual_needs_fastq_before_the_device(tmp_path):
    from kman_amd import engine
    from kman_amd.batcher import FastaBatcher

    fa = tmp_path / "in.fa"
    fa.write_bytes(b">r\nACGTACGT\n")
    gz = tmp_path / "in.fa.gz"
    import gzip

    with gzip.open(gz, "wb") as fh:
        fh.write(b">r\nACGTACGT\n")
    msg = "--min-qual needs fastq input"
    with pytest.raises(AssertionError, match=msg):
        engine.parse(_NoDevice(), b">r\nACGT\n", "auto", 20)
    with pytest.raises(AssertionError, match=msg):
        engine.parse(_NoDevice(), b"@r\nACGT\n+\nIIII\n", "fasta", 20)
    for path in (fa, gz):
        with pytest.raises(AssertionError, match=msg):
            engine.parse_file(_NoDevice(), str(path), "auto", 20)
    with pytest.raises(AssertionError, match=msg):
        engine.abundance_hist(b">r\nACGT\n", 3, dev=_NoDevice(), min_qual=20)
    with pytest.raises(AssertionError, match=msg):
        FastaBatcher(min_qual=20, device=_NoDevice()).do(str(fa), 3)


def test_parsed_n_masked_defaults_to_zero():
    import numpy as np

    from kman_amd.engine import Parsed

    p = Parsed(None, None, 0, 0, np.zeros(0, np.uint64), np.zeros(0, np.uint64), [], b"", np.zeros(1, np.uint64))
    assert p.n_masked == 0
