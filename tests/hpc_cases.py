"""`--hpc` test helper (not a conftest): a plain-Python statement of
kman_hpc_records, of the same compression applied to a FASTA / FASTQ text, and
of engine.hpc_spans (include/kman.h), independent of the code under test.

The rule on codes: base i is dropped exactly when i > 0, bits 2 and 3 of
code[i] are clear and (code[i - 1] & 7) == (code[i] & 7).  On text: within a
record, a character in ACGT (either case) that equals, case-insensitively, the
character before it is dropped; every other character is kept.
"""

from __future__ import annotations

import re

import numpy as np

_TERM = re.compile(rb"\r\n|\n|\r")


def dropped(code: int, prev: int) -> bool:
    return (code & 0x0C) == 0 and (prev & 7) == (code & 7)


def hpc_codes(codes, rec_seq):
    """(out, out_rec_seq, orig) of codes (n bytes, no pad) and a record table:
    the kept codes, per record the kept bases with an original index below its
    entry (entries clamped to n), and the original index of every kept base."""
    codes = [int(c) for c in codes]
    n = len(codes)
    out, orig = [], []
    before = [0] * (n + 1)  # before[i]: the kept bases with an original index < i
    for i, c in enumerate(codes):
        before[i] = len(out)
        if i > 0 and dropped(c, codes[i - 1]):
            continue
        out.append(c)
        orig.append(i)
    before[n] = len(out)
    out_rec = [before[min(int(p), n)] for p in rec_seq]
    return (np.asarray(out, dtype=np.uint8), np.asarray(out_rec, dtype=np.uint64),
            np.asarray(orig, dtype=np.uint64))


def hpc_seq(seq: str):
    """(compressed sequence, the original column of every kept character)."""
    out, cols = [], []
    for i, ch in enumerate(seq):
        if i > 0 and ch.upper() in "ACGT" and seq[i - 1].upper() == ch.upper():
            continue
        out.append(ch)
        cols.append(i)
    return "".join(out), cols


def text_records(text: bytes):
    """(header line without its first character, sequence) of every record of
    a FASTA (sequence lines joined) or a four-line FASTQ text."""
    lines = [ln.decode() for ln in _TERM.split(text)]
    recs = []
    if text[:1] == b"@":
        while lines and lines[-1] == "":
            lines.pop()
        for i in range(0, len(lines), 4):
            recs.append((lines[i][1:], "".join(lines[i + 1].split()) if i + 1 < len(lines) else ""))
        return recs
    for ln in lines:
        if ln.startswith(">"):
            recs.append((ln[1:], ""))
        elif recs:
            recs[-1] = (recs[-1][0], recs[-1][1] + "".join(ln.split()))
    return recs


def hpc_text(text: bytes) -> bytes:
    """A FASTA with the records' header lines (so the same names) and each
    sequence compressed; a record without bases is its header alone."""
    return "".join(">%s\n%s" % (h, hpc_seq(s)[0] + "\n" if s else "") for h, s in text_records(text)).encode()


def map_span(start: int, end: int, cols, length: int):
    """(START, END) of the original record for a span of the compressed one:
    cols = hpc_seq's columns, length = the original record's length.  END maps
    to the first column of the base after the stretch, or to the record's end,
    so the whole run of the stretch's last base lies inside; 0, 0 stays."""
    if end <= start:
        return 0, 0
    return cols[start], (cols[end] if end < len(cols) else length)


# ------------------------------------------------------------------ builders


def skewed_codes(n: int, seed: int, p=(0.7, 0.1, 0.1, 0.1), n_frac: float = 0.02, starts=()):
    """n codes whose base probabilities make long runs, a few N (4), bit 3 on
    index 0 and on every index of `starts`."""
    rng = np.random.default_rng(seed)
    c = rng.choice(4, size=n, p=p).astype(np.uint8)
    if n:
        c[rng.random(n) < n_frac] = 4
        c[0] |= 8
    for s in starts:
        if s < n:
            c[s] |= 8
    return c


def vary_homopolymers(seq: str, rng, frac: float = 0.5) -> str:
    """seq with the length of about `frac` of its runs of two or more equal
    bases changed by one (never to zero): the long-read error that --hpc is for."""
    out, i = [], 0
    while i < len(seq):
        j = i
        while j < len(seq) and seq[j] == seq[i]:
            j += 1
        ln = j - i
        if ln >= 2 and rng.random() < frac:
            ln += 1 if rng.random() < 0.5 else -1
        out.append(seq[i] * ln)
        i = j
    return "".join(out)
