"""FASTQ test helper (not a conftest): a pure-Python restatement of the strict
four-line FASTQ rules of kman_parse_fastq (include/kman.h), independent of the
code under test, and the builders of the test inputs.

The expected value of every FASTQ test is what the FASTA oracles
(np_oracle.parse_fasta, oracle/kman_oracle) give for ``fastq_to_fasta(text)``.
"""

from __future__ import annotations

import re

import numpy as np


def fastq_lines(text: bytes):
    """The lines of `text` (universal newlines) without the trailing empty
    ones, padded with empty lines to a multiple of four."""
    lines = re.split(rb"\r\n|\n|\r", text)
    while lines and lines[-1] == b"":
        lines.pop()
    while len(lines) % 4:
        lines.append(b"")
    return lines


def fastq_to_fasta(text: bytes) -> bytes:
    """The FASTA with the same records: ``>`` + the header line past its ``@``,
    then the sequence line.  AssertionError with kman_parse_fastq's messages
    for an input that breaks a rule."""
    lines = fastq_lines(text)
    if not lines:
        raise AssertionError("premature end of file or empty file")
    out = []
    for r in range(0, len(lines), 4):
        l0, l1, l2, l3 = lines[r:r + 4]
        rec = "FASTQ record %d: " % (r // 4 + 1)
        if l0[:1] != b"@":
            raise AssertionError(rec + "header line does not start with '@'")
        if l2[:1] != b"+":
            raise AssertionError(rec + "separator line does not start with '+'")
        if len(l3) != len(l1):
            raise AssertionError(rec + "quality length %d != sequence length %d" % (len(l3), len(l1)))
        out.append(b">" + l0[1:] + b"\n" + l1 + b"\n")
    return b"".join(out)


# ------------------------------------------------------------------ builders

_BASES = np.frombuffer(b"ACGTacgtN", dtype=np.uint8)
_QUAL = np.arange(ord("!"), ord("~") + 1, dtype=np.uint8)


def seq_of(rng, n: int, alphabet=_BASES) -> bytes:
    return alphabet[rng.integers(0, len(alphabet), n)].tobytes() if n else b""


def qual_of(rng, n: int, first: bytes = b"") -> bytes:
    """n quality bytes from all of ``!``..``~``; `first` forces the first byte."""
    q = _QUAL[rng.integers(0, len(_QUAL), n)].tobytes() if n else b""
    return (first + q[len(first):]) if n >= len(first) and first else q


def record(name: bytes, seq: bytes, qual: bytes, plus: bytes = b"+", nl: bytes = b"\n") -> bytes:
    return b"@" + name + nl + seq + nl + plus + nl + qual + nl


def mixed_reads(seed: int = 1, n_records: int = 300, nl: bytes = b"\n") -> bytes:
    """About n_records reads of lengths 0, 1, 20, 21, 22, 63, 64, 65, 150 and
    151 in random order: zero-length reads first, last and adjacent; quality
    lines that begin with ``@``, ``>`` and ``+``; ``+`` lines that repeat the
    name; headers with a description and a tab; bases from ACGTacgtN."""
    rng = np.random.default_rng(seed)
    lens = [0, 0] + [int(x) for x in rng.choice([0, 1, 20, 21, 22, 63, 64, 65, 150, 151], n_records - 5)] + [0, 0, 0]
    out = []
    for i, n in enumerate(lens):
        name = b"read%d" % i
        if i % 3 == 1:
            name += b" length=%d some description" % n
        if i % 7 == 2:
            name += b"\tafter a tab"
        first = (b"@", b">", b"+", b"")[i % 4]
        plus = b"+" + (name if i % 5 == 0 else b"")
        out.append(record(name, seq_of(rng, n), qual_of(rng, n, first), plus, nl))
    return b"".join(out)


def header_at(offset: int, seed: int = 2, read_len: int = 100) -> bytes:
    """Reads of which one has its ``@`` at byte `offset` exactly (the read
    before it is stretched to fit)."""
    rng = np.random.default_rng(seed)
    out, at, i = [], 0, 0
    assert offset >= 7
    while True:
        rec = record(b"r%d" % i, seq_of(rng, read_len), qual_of(rng, read_len))
        if at + len(rec) + 8 > offset:
            break
        out.append(rec)
        at += len(rec)
        i += 1
    # the filler read ends exactly at `offset`: 2 n + 7 bytes named "f", 2 n + 8 named "fx"
    gap = offset - at
    name, n = (b"f", (gap - 7) // 2) if gap % 2 else (b"fx", (gap - 8) // 2)
    out.append(record(name, seq_of(rng, n), qual_of(rng, n)))
    for j in range(3):
        out.append(record(b"edge%d" % j, seq_of(rng, read_len), qual_of(rng, read_len)))
    text = b"".join(out)
    assert text[offset:offset + 5] == b"@edge" and text[offset - 1:offset] == b"\n"
    return text


def long_reads(total: int, seed: int = 3, lo: int = 10_000, hi: int = 30_000) -> bytes:
    """About `total` bytes of reads of lo..hi bases."""
    rng = np.random.default_rng(seed)
    out, at, i = [], 0, 0
    acgt = _BASES[:4]
    while at < total:
        n = int(rng.integers(lo, hi))
        s = seq_of(rng, n, acgt)
        out.append(record(b"long%d" % i, s, qual_of(rng, n)))
        at += len(out[-1])
        i += 1
    return b"".join(out)


def short_reads(total: int = 2_000_000, seed: int = 4) -> bytes:
    """About `total` bytes of 25- to 150-base reads (ACGT with a few N)."""
    rng = np.random.default_rng(seed)
    alphabet = np.frombuffer(b"ACGT" * 30 + b"N", dtype=np.uint8)
    n_rec = total // 190
    lens = rng.integers(25, 151, n_rec)
    out = []
    for i, n in enumerate(lens.tolist()):
        out.append(record(b"sr%d/1 lane=%d" % (i, i % 8), seq_of(rng, n, alphabet), qual_of(rng, n)))
    return b"".join(out)
