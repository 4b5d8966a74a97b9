"""`kmer screen --reads-out` / `--trim` test helper (not a conftest): a
plain-Python statement of the bytes kman_cut_records writes (include/kman.h),
independent of the code under test, and the builders of the test inputs.  Lines
are split as fastq_cases.fastq_lines splits them.
"""

from __future__ import annotations

import re

import numpy as np

STRIP = b" \t\n\r\v\f\x1c\x1d\x1e\x1f"  # what the parsers right-strip from a sequence line
_TERM = re.compile(rb"\r\n|\n|\r")


def clamp_offsets(off, n_bytes: int) -> list:
    return [min(int(x), n_bytes) for x in off]


def records_of(text: bytes, off) -> list:
    """The records of n + 1 offsets: record r is [off[r], off[r + 1]), every
    offset clamped to the text, a descending pair empty."""
    o = clamp_offsets(off, len(text))
    return [text[o[r]:max(o[r], o[r + 1])] for r in range(len(o) - 1)]


def record_bytes(text: bytes, off, r: int) -> bytes:
    return records_of(text, off[r:r + 2])[0]


def record_lines(rec: bytes) -> list:
    """The record's first four raw lines without their terminators; a line the
    record does not have is empty."""
    return (_TERM.split(rec) + [b""] * 4)[:4]


def cols_of(l2: bytes) -> list:
    """The raw columns of a sequence line that got a code."""
    body = l2.rstrip(STRIP)
    return [c for c in range(len(body)) if body[c] not in b" \r"]


def cut_whole(text: bytes, off, keep=None) -> bytes:
    return b"".join(rec for r, rec in enumerate(records_of(text, off)) if keep is None or keep[r])


def trimmed_record(rec: bytes, start: int, end: int) -> bytes:
    """One record cut to columns [start, end): b"" when nothing is written."""
    if not rec:
        return b""
    l1, l2, l3, l4 = record_lines(rec)
    cols = cols_of(l2)
    end = min(int(end), len(cols))
    start = int(start)
    if start >= end:
        return b""
    c0, c1 = cols[start], cols[end - 1] + 1
    return l1 + b"\n" + l2[c0:c1] + b"\n" + l3 + b"\n" + l4[c0:c1] + b"\n"


def cut_trimmed(text: bytes, off, start, end, keep=None) -> bytes:
    return b"".join(trimmed_record(rec, start[r], end[r])
                    for r, rec in enumerate(records_of(text, off)) if keep is None or keep[r])


# ------------------------------------------------------------------ builders


def fastq_offsets(text: bytes) -> list:
    """The byte offset of every record's ``@`` (every fourth line start, as
    fastq_cases.fastq_lines counts lines) followed by len(text)."""
    starts, at = [], 0
    for m in _TERM.finditer(text):
        starts.append(at)
        at = m.end()
    if at < len(text):
        starts.append(at)
    while starts and not text[starts[-1]:].strip(b"\r\n"):  # (trailing empty lines)
        starts.pop()
    return starts[::4] + [len(text)]


def fasta_offsets(text: bytes) -> list:
    """The byte offset of every ``>`` that starts a line, followed by len(text)."""
    return [m.start() for m in re.finditer(rb"(?:^|(?<=[\r\n]))>", text)] + [len(text)]


def byte_records(lengths, seed: int = 1, gap: int = 0, first: int = 0):
    """(text, offsets): records of the given byte lengths made of random
    printable bytes, after `first` bytes that belong to no record; every record
    is followed by `gap` more bytes of its own (lengths + gap each)."""
    rng = np.random.default_rng(seed)
    body = rng.integers(33, 127, first + sum(lengths) + gap * len(lengths), dtype=np.uint8).tobytes()
    off, at = [], first
    for n in lengths:
        off.append(at)
        at += n + gap
    return body[:at], off + [at]


# the hand-written trim cases: (record text, START, END, expected bytes)
HAND_TRIM = [
    # CRLF
    (b"@r1 d\r\nACGTACGT\r\n+\r\nIIIIHHHH\r\n", 2, 6, b"@r1 d\nGTAC\n+\nIIHH\n"),
    # lone CR
    (b"@r2\rACGTA\r+r2\r!!#$%\r", 1, 4, b"@r2\nCGT\n+r2\n!#$\n"),
    # blanks inside and whitespace after the sequence: cols = 0 1 3 4 6, quality cut by the same raw columns
    (b"@r3\nAC GT A \t\n+\n012345678\n", 1, 4, b"@r3\nC GT\n+\n1234\n"),
    (b"@r3\nAC GT A \t\n+\n012345678\n", 0, 5, b"@r3\nAC GT A\n+\n0123456\n"),
    # the last record without a final newline
    (b"@r4\nACGT\n+\nabcd", 1, 3, b"@r4\nCG\n+\nbc\n"),
    # START = 0, END = len, a one-base stretch
    (b"@r5\nACGTN\n+\nabcde\n", 0, 2, b"@r5\nAC\n+\nab\n"),
    (b"@r5\nACGTN\n+\nabcde\n", 3, 5, b"@r5\nTN\n+\nde\n"),
    (b"@r5\nACGTN\n+\nabcde\n", 0, 5, b"@r5\nACGTN\n+\nabcde\n"),
    (b"@r5\nACGTN\n+\nabcde\n", 2, 3, b"@r5\nG\n+\nc\n"),
    # END beyond the kept bytes is clamped; START == END and START past them write nothing
    (b"@r6\nACGT  \n+\nabcdef\n", 2, 99, b"@r6\nGT\n+\ncd\n"),
    (b"@r6\nACGT\n+\nabcd\n", 2, 2, b""),
    (b"@r6\nACGT\n+\nabcd\n", 4, 9, b""),
    # an empty sequence line, and a padded last record without its last lines
    (b"@r7\n\n+\n\n", 0, 1, b""),
    (b"@r8\nACG", 1, 3, b"@r8\nCG\n\n\n"),
]


def planted_reads(seed: int = 11, n_reads: int = 40, read_len: int = 60, copies: int = 4, genome_len: int = 400):
    """(fastq text, [(name, seq)]) : reads of one random genome, `copies` at
    every start, every third read with one base changed near its middle, so
    that screened against themselves with --solid 2 most reads have a stretch
    shorter than the read."""
    rng = np.random.default_rng(seed)
    genome = rng.integers(0, 4, genome_len)
    out, recs = [], []
    at = 0
    for i in range(n_reads):
        if i % copies == 0:
            at = int(rng.integers(0, genome_len - read_len))
        s = genome[at:at + read_len].copy()
        if i % 3 == 0:
            s[read_len // 2 + i % 5] ^= 1 + i % 3
        seq = bytes(b"ACGT"[x] for x in s)
        qual = bytes(33 + int(x) for x in rng.integers(0, 60, read_len))
        if qual[:1] == b"@":
            qual = b"I" + qual[1:]
        name = b"p%d" % i
        out.append(b"@" + name + b" x\n" + seq + b"\n+\n" + qual + b"\n")
        recs.append((name.decode(), seq.decode()))
    return b"".join(out), recs
