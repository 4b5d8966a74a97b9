"""`kmer screen` test helper (not a conftest): a plain-Python statement of
kman_screen_records / engine.screen_keep / kman_format_screen (include/kman.h),
independent of the code under test, and the builders of the record layouts.

Records are ``(name, sequence)`` pairs of str.  A window is valid when its k
characters, upper-cased, are all in ACGT; it never crosses a record.  The
canonical k-mer is the smaller of the window and its reverse complement, as
strings (A < C < G < T is also the order of the 2-bit keys).
"""

from __future__ import annotations

import numpy as np

_COMP = str.maketrans("ACGT", "TGCA")
_CODE = {"A": 0, "C": 1, "G": 2, "T": 3}
MASK64 = (1 << 64) - 1


def revcomp(s: str) -> str:
    return s.translate(_COMP)[::-1]


def key_of(kmer: str) -> int:
    v = 0
    for ch in kmer:
        v = (v << 2) | _CODE[ch]
    return v


def windows(seq: str, k: int, canonical: bool = False):
    """The k-mers of the valid windows of one record, in order."""
    up = seq.upper()
    out = []
    for i in range(len(up) - k + 1):
        w = up[i:i + k]
        if all(ch in _CODE for ch in w):
            out.append(min(w, revcomp(w)) if canonical else w)
    return out


def table_of(records, k: int, canonical: bool = False, min_count: int = 1, max_count=None) -> dict:
    """k-mer -> count over all records, within [min_count, max_count]."""
    t = {}
    for _, seq in records:
        for w in windows(seq, k, canonical):
            t[w] = t.get(w, 0) + 1
    return {w: c for w, c in t.items() if c >= min_count and (max_count is None or c <= max_count)}


def table_rows(table: dict, count_bytes: int = 4):
    """The table as key-sorted rows: (u64 keys, counts)."""
    rows = sorted((key_of(w), c) for w, c in table.items())
    keys = np.asarray([r[0] for r in rows], dtype=np.uint64)
    counts = np.asarray([r[1] for r in rows], dtype=np.uint32 if count_bytes == 4 else np.uint64)
    return keys, counts


def stats(records, k: int, table: dict, canonical: bool = False) -> np.ndarray:
    """(windows, hits, count sum modulo 2^64) per record, an (n, 3) u64 array."""
    out = np.zeros((len(records), 3), dtype=np.uint64)
    for r, (_, seq) in enumerate(records):
        ws = windows(seq, k, canonical)
        hit = [table[w] for w in ws if w in table]
        out[r] = (len(ws), len(hit), sum(hit) & MASK64)
    return out


def keep(st, min_hits: int = 0, min_frac: float = 0.0, invert: bool = False):
    """hits >= min_hits and hits >= min_frac * windows, flipped when invert."""
    res = []
    for w, h, _ in np.asarray(st).tolist():
        ok = float(h) >= min_hits and float(h) >= min_frac * float(w)
        res.append(bool(ok) != bool(invert))
    return res


def lines(records, st, kept=None) -> bytes:
    out = []
    for r, (name, _) in enumerate(records):
        if kept is None or kept[r]:
            w, h, s = (int(x) for x in st[r])
            out.append(("%s\t%d\t%d\t%d\n" % (name, w, h, s)).encode())
    return b"".join(out)


def fasta(records) -> bytes:
    """One line per sequence; a record without bases is its header alone."""
    return "".join(">%s\n%s" % (n, s + "\n" if s else "") for n, s in records).encode()


def fasta_records(text: bytes):
    """The records of a FASTA text: name = the header's first word, sequence =
    its lines joined."""
    recs = []
    for block in text.decode().split(">")[1:]:
        head, _, body = block.partition("\n")
        recs.append((head.rstrip().split(" ")[0], "".join(body.split("\n"))))
    return recs


def codes_of(records):
    """The parsers' device layout of the records: (codes + 64 bytes of padding
    (code 4), rec_seq, n_bases).  Code: bits 0-1 the base, 4 = not ACGT, bit 3
    on a record's first base."""
    codes, rec_seq = [], []
    for _, seq in records:
        rec_seq.append(len(codes))
        for i, ch in enumerate(seq.upper()):
            codes.append(_CODE.get(ch, 4) | (8 if i == 0 else 0))
    n = len(codes)
    return np.asarray(codes + [4] * 64, dtype=np.uint8), np.asarray(rec_seq, dtype=np.uint64), n


# ------------------------------------------------------------------ builders


def rand_seq(rng, n: int) -> str:
    return "".join("ACGT"[i] for i in rng.integers(0, 4, n)) if n else ""


def records_of(lengths, seed: int = 1, prefix: str = "r"):
    rng = np.random.default_rng(seed)
    return [("%s%d" % (prefix, i), rand_seq(rng, int(n))) for i, n in enumerate(lengths)]


def with_n(seq: str, spans) -> str:
    """seq with [a, b) replaced by N (lower-case n in odd spans) for every span."""
    s = list(seq)
    for j, (a, b) in enumerate(spans):
        for i in range(a, min(b, len(s))):
            s[i] = "n" if j % 2 else "N"
    return "".join(s)


def layouts(k: int, T: int, cap: int) -> dict:
    """name -> record lengths.  T: the kernel's tile in windows; cap: the
    rec_seq entries of a tile it stages in LDS."""
    return {
        "reads150": [150] * 40 + [37],                        # two tiles; n_bases no multiple of 16
        "tiny_run": [0, 1, k - 1, k, k + 1] * 3 + [150, 0, 1, k],
        "equal_entries": [0, 0, 0, 200, 0, 0, 300, 1, 0, 0, 0],  # at the start, in the middle, as the last records
        "boundary_T": [T - 1, 1, 1, 50, T - 53, k + 2],       # record boundaries at base T - 1, T, T + 1 (and 2 T)
        "spanning": [5, 7, 3 * T + 100, 9, 4, k + 5],         # one record over more than 3 T bases
        "many_small": [150, 150] + [1, 0] * cap + [150, 150] + [k + 3] * 20,   # > cap entries in tile 0
        "many_small_carry": [T - 10, 150] + [1, 0, 0] * cap + [150, 2 * k],    # > cap in tile 1, after a carry-in
        "only_small": [1, 0] * (cap + 5),                     # > cap entries, no window at all
        "bases_k_minus_1": [k - 1],
        "bases_k": [k],
        "two_short": [k - 1, k - 1],
    }


def n_run_records(k: int, T: int, seed: int = 3):
    """One record over two tiles with N runs on and around the tile boundary,
    one wholly N, one lower-case."""
    rng = np.random.default_rng(seed)
    a = with_n(rand_seq(rng, 2 * T + 77), [(T - 3, T + 2), (T + k, T + k + 1), (5, 6), (2 * T - 1, 2 * T + 1)])
    return [("nrun", a), ("alln", "N" * (k + 4)), ("lower", rand_seq(rng, 90).lower()), ("tail", rand_seq(rng, 61))]
