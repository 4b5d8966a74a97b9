"""Read pairs in plain Python and numpy: what kman_zip_records writes, the pair
name rule, the pair-joint statistics, median, selection and the two TSV
layouts of `kmer screen --mate` / `--interleaved`.  The statements the GPU
tests compare against; nothing here imports the package."""

from __future__ import annotations

import numpy as np

import median_cases as mc
import screen_cases as sc

PAD = 64  # pad bytes of value 4 after the codes


# ------------------------------------------------------------------------ zip


def zip_codes(codes1, rec_seq1, n1: int, codes2, rec_seq2, n2: int):
    """(codes + 64 pad bytes, rec_seq) of two code buffers zipped by record:
    mate 1 of pair i directly before mate 2 of pair i, pairs in order, every
    byte verbatim; entry 2i of rec_seq starts mate 1 of pair i, entry 2i + 1
    its mate 2.  Record r of a source is [rec_seq[r], rec_seq[r + 1]), the last
    one runs to n.  No pairs: the pad alone."""
    c1, c2 = np.asarray(codes1, np.uint8), np.asarray(codes2, np.uint8)
    r1, r2 = [int(x) for x in rec_seq1] + [n1], [int(x) for x in rec_seq2] + [n2]
    assert len(r1) == len(r2)
    out, rec = [], []
    at = 0
    for i in range(len(r1) - 1):
        for c, a, b in ((c1, r1[i], r1[i + 1]), (c2, r2[i], r2[i + 1])):
            rec.append(at)
            out.append(c[a:b])
            at += b - a
    out.append(np.full(PAD, 4, np.uint8))
    return np.concatenate(out), np.asarray(rec, np.uint64)


def zip_records(recs1, recs2):
    """The mate view as a record list: R1[0], R2[0], R1[1], R2[1], .."""
    assert len(recs1) == len(recs2)
    return [r for pair in zip(recs1, recs2) for r in pair]


def mate_codes(lengths, seed: int, masked: bool = True):
    """(codes without pad, rec_seq, n) of records of the given lengths as a
    parser writes them: random bases, bit 3 on a record's first code, and,
    `masked`, some codes with bit 2 set (an N, or a base that -q masked)."""
    rng = np.random.default_rng(seed)
    n = int(sum(lengths))
    codes = rng.integers(0, 4, n).astype(np.uint8)
    if masked and n:
        codes[rng.integers(0, n, max(1, n // 9))] = 4
    rec, at = [], 0
    for ln in lengths:
        rec.append(at)
        if ln:
            codes[at] |= 8
        at += int(ln)
    return codes, np.asarray(rec, np.uint64), n


# ---------------------------------------------------------------------- names


def pair_key(name: bytes) -> bytes:
    """A record name with one trailing /1 or /2 removed."""
    return name[:-2] if name[-2:] in (b"/1", b"/2") else name


def first_name_mismatch(names1, names2) -> int:
    """The 0-based index of the first pair whose names differ, -1: none."""
    for i, (a, b) in enumerate(zip(names1, names2)):
        if pair_key(a) != pair_key(b):
            return i
    return -1


# HAND_NAMES: (name of mate 1, name of mate 2, the pair is accepted)
HAND_NAMES = [
    (b"r1/1", b"r1/2", True),
    (b"r1", b"r1", True),
    (b"r1/1", b"r1", True),       # a suffix on one side only
    (b"r1", b"r1/2", True),
    (b"r1/2", b"r1/1", True),     # either suffix on either side
    (b"r1/1", b"r11/2", False),
    (b"r1/1", b"r2/2", False),
    (b"r1/3", b"r1/2", False),    # /3 is part of the name
    (b"r1/1/1", b"r1/1", False),  # one suffix is removed, not two: r1/1 and r1
    (b"/1", b"/2", True),         # an empty key on both sides
    (b"", b"", True),
    (b"1", b"2", False),          # no slash: nothing is removed
]


# ----------------------------------------------------------------- statistics


def pair_stats(st1, st2) -> np.ndarray:
    """The pair-joint (windows, hits, sum modulo 2^64): the sums of the mates' rows."""
    a, b = np.asarray(st1, np.uint64).reshape(-1, 3), np.asarray(st2, np.uint64).reshape(-1, 3)
    return a + b  # (u64 arithmetic wraps)


def pair_medians(recs1, recs2, k: int, table: dict, canonical: bool = False) -> list:
    """The lower median over the union of both mates' window counts."""
    return [mc.quantile(mc.window_words([a], k, table, canonical) + mc.window_words([b], k, table, canonical))
            for a, b in zip(recs1, recs2)]


def pair_keep(st, med=None, span1=None, span2=None, min_hits: int = 0, min_frac: float = 0.0, invert: bool = False,
              min_median=None, max_median=None, min_solid_len=None) -> list:
    """The pairs that are written: the joint numbers pass min_hits, min_frac
    and the median bounds, and both mates' stretches have min_solid_len bases;
    the others under invert."""
    res = []
    for r, (w, h, _) in enumerate(np.asarray(st).tolist()):
        ok = float(h) >= min_hits and float(h) >= min_frac * float(w)
        if min_median is not None:
            ok = ok and int(med[r]) >= min_median
        if max_median is not None:
            ok = ok and int(med[r]) <= max_median
        if min_solid_len is not None:
            ok = ok and all(int(s[r][1]) - int(s[r][0]) >= min_solid_len for s in (span1, span2))
        res.append(bool(ok) != bool(invert))
    return res


def pair_lines(names, st, med=None, span1=None, span2=None, kept=None) -> bytes:
    """NAME K-MERS HITS SUM [MEDIAN] [START END START2 END2], one line per
    written pair; NAME is mate 1's name as READS has it."""
    out = []
    for r, name in enumerate(names):
        if kept is not None and not kept[r]:
            continue
        cols = [name if isinstance(name, str) else name.decode()] + [str(int(x)) for x in st[r]]
        if med is not None:
            cols.append(str(int(med[r])))
        if span1 is not None:
            cols += [str(int(x)) for x in (span1[r][0], span1[r][1], span2[r][0], span2[r][1])]
        out.append("\t".join(cols) + "\n")
    return "".join(out).encode()


def fastq(records, suffix: str = "", qual: str = "I") -> bytes:
    """Four-line FASTQ of (name, sequence) records, `suffix` appended to every name."""
    return "".join("@%s%s\n%s\n+\n%s\n" % (n, suffix, s, qual * len(s)) for n, s in records).encode()


def interleave_fastq(records1, records2) -> bytes:
    return b"".join(fastq([a], "/1") + fastq([b], "/2") for a, b in zip(records1, records2))
