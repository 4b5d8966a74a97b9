"""FASTQ input on the CPU: the test restatement's known answers, format
sniffing, the vectorised record names, the ``--format`` option of every
command and the solo-rank route under a one-process-per-GPU launch."""

from __future__ import annotations

import numpy as np
import pytest

import fastq_cases as fq


def test_fastq_to_fasta_known_answers():
    assert fq.fastq_to_fasta(b"@a x\nACGT\n+\nIIII\n@b\nGG\n+b\n!!\n") == b">a x\nACGT\n>b\nGG\n"
    # a zero-length last read, with and without its last lines
    assert fq.fastq_to_fasta(b"@a\nAC\n+\nII\n@r\n\n+\n\n") == b">a\nAC\n>r\n\n"
    assert fq.fastq_to_fasta(b"@r\n\n+\n") == b">r\n\n"
    assert fq.fastq_to_fasta(b"@r\n\n+") == b">r\n\n"
    # \r\n and a lone \r end a line
    assert fq.fastq_to_fasta(b"@a\r\nACGT\r\n+\r\nIIII\r\n") == b">a\nACGT\n"
    assert fq.fastq_to_fasta(b"@a\rAC\r+\rII\r") == b">a\nAC\n"
    # no final newline; five trailing blank lines
    assert fq.fastq_to_fasta(b"@a\nACGT\n+\nIIII") == b">a\nACGT\n"
    assert fq.fastq_to_fasta(b"@a\nACGT\n+\nIIII\n\n\n\n\n\n") == b">a\nACGT\n"
    # quality lines that look like headers; what follows '+' is ignored
    assert fq.fastq_to_fasta(b"@a\nAC\n+a\n@>\n@b\nGT\n+\n+@\n") == b">a\nAC\n>b\nGT\n"
    # spaces inside the sequence line count for the length rule
    assert fq.fastq_to_fasta(b"@a\nA C \n+\nIIII\n") == b">a\nA C \n"


@pytest.mark.parametrize("text, msg", [
    (b"", "premature end of file or empty file"),
    (b"\n\r\n\n", "premature end of file or empty file"),
    (b"@a\nA\n+\nI\n@b\nA\n+\nI\nc\nA\n+\nI\n", "FASTQ record 3: header line does not start with '@'"),
    (b"\n@a\nA\n+\nI\n", "FASTQ record 1: header line does not start with '@'"),
    (b"@a\nA\n+\nI\n@b\nA\n-\nI\n", "FASTQ record 2: separator line does not start with '\\+'"),
    (b"@a\nACGTACGT\n+\nIIIIIII\n", "FASTQ record 1: quality length 7 != sequence length 8"),
    (b"@r", "FASTQ record 1: separator line does not start with '\\+'"),
    (b"@a\nA\n+\nI\n@b\n", "FASTQ record 2: separator line does not start with '\\+'"),
    (b"@a\nA\n+\nI\n@b\nAC\n", "FASTQ record 2: separator line does not start with '\\+'"),
    (b"@a\nA\n+\nI\n@b\nAC\n+\n", "FASTQ record 2: quality length 0 != sequence length 2"),
    (b"@a\nACGT\nACGT\n+\nIIII\nIIII\n", "FASTQ record 1: separator line does not start with '\\+'"),
    (b">a\nACGT\n", "FASTQ record 1: header line does not start with '@'"),
])
def test_fastq_to_fasta_errors(text, msg):
    with pytest.raises(AssertionError, match=msg):
        fq.fastq_to_fasta(text)


def test_builders_are_valid_fastq():
    for text in (fq.mixed_reads(), fq.mixed_reads(nl=b"\r\n"), fq.header_at(63), fq.header_at(16385),
                 fq.short_reads(50_000), fq.long_reads(100_000)):
        assert fq.fastq_to_fasta(text).startswith(b">")
    for off in (63, 64, 65, 16383, 16384, 16385):
        assert fq.header_at(off)[off:off + 6] == b"@edge0"


def test_sniff_format():
    from kman_amd.engine import sniff_format

    assert sniff_format(b"@r1\nACGT\n+\nIIII\n") == "fastq"
    assert sniff_format(b"\n\r\n\r@r1\nACGT\n+\nIIII\n") == "fastq"
    assert sniff_format(b">r1\nACGT\n") == "fasta"
    assert sniff_format(b";comment\n>r1\nACGT\n") == "fasta"
    assert sniff_format(b"\n\n>r1\nACGT\n") == "fasta"
    assert sniff_format(b" @r1\n") == "fasta"
    assert sniff_format(b"") == "fasta" and sniff_format(b"\n\n") == "fasta"


def test_sniff_file(tmp_path):
    import gzip

    from kman_amd.engine import sniff_file

    (tmp_path / "a.fq").write_bytes(b"\n" * 200_000 + b"@r\nA\n+\nI\n")
    (tmp_path / "b.fa").write_bytes(b"\n" * 200_000 + b">r\nA\n")
    (tmp_path / "e.fq").write_bytes(b"")
    with gzip.open(tmp_path / "c.fq.gz", "wb") as fh:
        fh.write(b"@r\nA\n+\nI\n")
    assert sniff_file(str(tmp_path / "a.fq")) == "fastq" and sniff_file(str(tmp_path / "b.fa")) == "fasta"
    assert sniff_file(str(tmp_path / "c.fq.gz")) == "fastq" and sniff_file(str(tmp_path / "e.fq")) == "fasta"


def _headers(seed: int, n: int):
    rng = np.random.default_rng(seed)
    words = [b"read", b"x", b"length=151", b"1:N:0:ACGT", b"caf\xc3\xa9", b"\xff\xfe", b"a\tb", b"\x0b", b"\x1c",
             b"\x0c", b"q" * 70, b"w" * 300, b"", b"\xc2\xa0", b"\xe2\x80\x83"]
    seps = [b" ", b"  ", b"\t", b" \t ", b""]
    out = []
    for i in range(n):
        parts = [words[j] for j in rng.integers(0, len(words), int(rng.integers(0, 5)))]
        h = b""
        for p in parts:
            h += p + seps[int(rng.integers(0, len(seps)))]
        if i % 9 == 0:
            h = b""  # an empty name
        if i % 11 == 0:
            h = b" " + h  # a title that begins with a space
        if i % 13 == 0:
            h += b"   "  # trailing spaces
        out.append(h)
    return out


@pytest.mark.parametrize("nl", [b"\n", b"\r\n", b"\r"])
def test_vectorised_names_equal_title_name(nl, monkeypatch):
    from kman_amd import engine

    heads = _headers(7, 2000)
    text, hdr = b"", []
    for h in heads:
        hdr.append(len(text))
        text += b"@" + h + nl + b"ACGT" + nl + b"+" + nl + b"IIII" + nl
    hdr.append(len(text))
    text += b"@last\xc3\xa9 header at the end"  # no terminator
    hdr = np.asarray(hdr, dtype=np.uint64)
    want = [engine._title_name(text, int(h)) for h in hdr]
    for rows in (1 << 16, 300):  # one numpy block, several
        monkeypatch.setattr(engine.parsed, "_NAME_ROWS", rows)
        blob, off = engine.fastq_names(text, hdr)
        names = engine.BlobNames(blob, off)
        assert list(names) == want and names == want and len(names) == len(want)
        assert blob == b"".join(want) and off[-1] == len(blob) and names[-1] == want[-1] and names[3:5] == want[3:5]
    # a header at the end of the text that is plain ASCII
    t2 = b"@a b\nA\n+\nI\n@zz"
    blob, off = engine.fastq_names(t2, np.asarray([0, 11], dtype=np.uint64))
    assert blob == b"azz" and off.tolist() == [0, 1, 3]


@pytest.mark.parametrize("cmd", ["count", "uniq", "batch", "hist"])
def test_commands_take_format_option(cmd, tmp_path):
    from click.testing import CliRunner

    from kman_amd.scripts.kmer import main

    run = CliRunner()
    r = run.invoke(main, [cmd, "--help"])
    assert r.exit_code == 0 and "--format" in r.output and "-f" in r.output and "fastq" in r.output
    assert "INPUT fasta or fastq file, plain or gzipped" in " ".join(r.output.split())
    src = tmp_path / "in.fq"
    src.write_bytes(b"@r\nACGT\n+\nIIII\n")
    for flag in ("-f", "--format"):
        r = run.invoke(main, [cmd, str(src), str(tmp_path / "out"), "3", flag, "bam"])
        assert r.exit_code == 2 and "bam" in r.output and not (tmp_path / "out").exists()
    # a good value passes the option parser: the command then stops at k = 1,
    # before any device work
    for val in ("auto", "fasta", "fastq"):
        r = run.invoke(main, [cmd, str(src), str(tmp_path / "out"), "1", "-f", val])
        assert r.exit_code != 2
        if cmd == "hist":
            assert isinstance(r.exception, AssertionError) and "k must be >= 1" in str(r.exception)


def test_multi_gpu_fastq_is_solo_rank(tmp_path, monkeypatch):
    from kman_amd.scripts.kmer import _multi_gpu

    fqp, fap, blank = tmp_path / "in.fq", tmp_path / "in.fa", tmp_path / "blank.fq"
    fqp.write_bytes(b"@r\nACGT\n+\nIIII\n")
    fap.write_bytes(b">r\nACGT\n")
    blank.write_bytes(b"\n\n@r\nACGT\n+\nIIII\n")
    for v in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "KMAN_DIST"):
        monkeypatch.delenv(v, raising=False)
    assert _multi_gpu(21, None, "SEQ_COUNT", str(fqp), "auto") is False  # no launch
    monkeypatch.setenv("WORLD_SIZE", "4")
    for rank, solo in ((0, False), (2, None)):
        monkeypatch.setenv("RANK", str(rank))
        monkeypatch.setenv("LOCAL_RANK", str(rank))
        assert _multi_gpu(21, None, "SEQ_COUNT", str(fqp), "auto") is solo
        assert _multi_gpu(21, None, "UNIQUE", str(blank), "auto") is solo
        assert _multi_gpu(21, None, "SEQ_COUNT", str(fap), "fastq") is solo
        # FASTA input: what it returned before there was a format
        assert _multi_gpu(21, None, "SEQ_COUNT", str(fap), "auto") is True
        assert _multi_gpu(21, None, "SEQ_COUNT", str(fqp), "fasta") is True
        assert _multi_gpu(21, None, "UNIQUE") is True and _multi_gpu(1, None, "SEQ_COUNT", str(fqp)) is True
        assert _multi_gpu(33, None, "SEQ_COUNT", str(fap)) is solo
        assert _multi_gpu(21, "dir", "SEQ_COUNT", str(fap)) is solo
        assert _multi_gpu(21, None, "VEC_COUNT", str(fap)) is solo


def test_hist_fastq_solo_rank_returns_early(tmp_path, monkeypatch):
    """`kmer hist` of a FASTQ under a launch: a rank other than 0 returns
    before any device work."""
    from kman_amd.scripts.kmer import main

    src = tmp_path / "in.fq"
    src.write_bytes(b"@r\nACGT\n+\nIIII\n")
    monkeypatch.delenv("KMAN_DIST", raising=False)
    monkeypatch.setenv("WORLD_SIZE", "2")
    monkeypatch.setenv("RANK", "1")
    monkeypatch.setenv("LOCAL_RANK", "1")
    main(["hist", str(src), str(tmp_path / "h.txt"), "21"], standalone_mode=False)
    assert not (tmp_path / "h.txt").exists()


def test_native_signature_and_header():
    import os

    from conftest import ROOT
    from kman_amd import _native

    assert _native.SIGNATURES["kman_parse_fastq"] == _native.SIGNATURES["kman_parse_fasta"]
    with open(os.path.join(ROOT, "include", "kman.h")) as fh:
        assert "int kman_parse_fastq(kman_ctx *ctx" in fh.read()
