"""Set-operation test helper (not a conftest): a plain-numpy statement of the
eight ops of kman_match_counts (include/kman.h) and of the three set
operations of engine.set_op / `kmer sets`, by np.searchsorted, independent of
the code under test; the same set arithmetic on the text lines of two `count`
outputs, by Python dicts; and the key patterns of the GPU tests."""

from __future__ import annotations

import numpy as np

MATCH_OPS = ("right", "left", "min", "max", "sum", "absent", "any_sum", "any_max")  # in the order of KMAN_MATCH_*
SET_COUNTS = {"intersect": ("left", "right", "min", "max", "sum"), "subtract": ("left",), "union": ("sum", "max")}
U32_MAX = (1 << 32) - 1
U64_MAX = (1 << 64) - 1


def lookup(ak: np.ndarray, bk: np.ndarray, bc: np.ndarray):
    """(matched, cb as u64): for every key of ak, whether bk (strictly
    ascending) holds it and the count of that row, 0 when it does not."""
    ak = np.asarray(ak, np.uint64)
    bk = np.asarray(bk, np.uint64)
    if len(bk) == 0:
        return np.zeros(len(ak), bool), np.zeros(len(ak), np.uint64)
    j = np.searchsorted(bk, ak)
    jj = np.minimum(j, len(bk) - 1)
    hit = (j < len(bk)) & (bk[jj] == ak)
    return hit, np.where(hit, np.asarray(bc).astype(np.uint64)[jj], np.uint64(0))


def _add_sat(a: np.ndarray, b: np.ndarray) -> np.ndarray:
    s = a + b  # (wraps)
    return np.where(s < a, np.uint64(U64_MAX), s)


def match(ak, ac, bk, bc, op: str, out_bytes: int = 4) -> np.ndarray:
    """out[i] of kman_match_counts, in the dtype of out_bytes."""
    hit, cb = lookup(ak, bk, bc)
    ca = np.asarray(ac).astype(np.uint64)
    zero = np.uint64(0)
    r = {
        "right": lambda: cb,
        "left": lambda: np.where(hit, ca, zero),
        "min": lambda: np.where(hit, np.minimum(ca, cb), zero),
        "max": lambda: np.where(hit, np.maximum(ca, cb), zero),
        "sum": lambda: np.where(hit, _add_sat(ca, cb), zero),
        "absent": lambda: np.where(hit, zero, ca),
        "any_sum": lambda: _add_sat(ca, cb),
        "any_max": lambda: np.maximum(ca, cb),
    }[op]()
    if out_bytes == 4:
        return np.minimum(r, np.uint64(U32_MAX)).astype(np.uint32)
    return r.astype(np.uint64)


def set_op(ak, ac, bk, bc, op: str, counts=None, lo: int = 1, hi=None, out_bytes: int = 4):
    """(keys, counts) of the set operation, rows with a count in [max(1, lo), hi]."""
    counts = counts or SET_COUNTS[op][0]
    assert counts in SET_COUNTS[op]
    ak = np.asarray(ak, np.uint64)
    bk = np.asarray(bk, np.uint64)
    if op == "intersect":
        k, c = ak, match(ak, ac, bk, bc, counts, out_bytes)
    elif op == "subtract":
        k, c = ak, match(ak, ac, bk, bc, "absent", out_bytes)
    else:
        ca = match(ak, ac, bk, bc, "any_" + counts, out_bytes)
        only_b = match(bk, bc, ak, ac, "absent", out_bytes)
        kb = only_b != 0
        k = np.concatenate([ak, bk[kb]])
        c = np.concatenate([ca, only_b[kb]])
        order = np.argsort(k, kind="stable")
        k, c = k[order], c[order]
    keep = (c >= max(1, lo)) & (c != 0)
    if hi is not None:
        keep &= c <= hi
    return k[keep], c[keep]


# ------------------------------------------------------------ text lines

_CODE = {c: i for i, c in enumerate(b"ACGT")}


def lines_to_rows(text: bytes, k: int):
    """(keys, counts u64) of a `count` output's "SEQ\\tN" lines (2 bits per base, first base highest)."""
    keys, counts = [], []
    for line in text.splitlines():
        seq, n = line.split(b"\t")
        assert len(seq) == k
        v = 0
        for ch in seq:
            v = (v << 2) | _CODE[ch]
        keys.append(v)
        counts.append(int(n))
    return np.asarray(keys, np.uint64), np.asarray(counts, np.uint64)


def rows_to_lines(keys, counts, k: int) -> bytes:
    out = []
    for key, n in zip(np.asarray(keys).tolist(), np.asarray(counts).tolist()):
        out.append(bytes(b"ACGT"[(key >> (2 * (k - 1 - j))) & 3] for j in range(k)) + b"\t%d\n" % n)
    return b"".join(out)


def lines_set_op(a_text: bytes, b_text: bytes, op: str, counts=None, lo: int = 1, hi=None) -> bytes:
    """The set operation on two `count` outputs by dicts of their lines: the
    expected `kmer sets` output (sequences in ascending order: A < C < G < T is
    the byte order too)."""
    counts = counts or SET_COUNTS[op][0]
    assert counts in SET_COUNTS[op]
    a = {s: int(n) for s, n in (ln.split(b"\t") for ln in a_text.splitlines())}
    b = {s: int(n) for s, n in (ln.split(b"\t") for ln in b_text.splitlines())}
    f = {"left": lambda x, y: x, "right": lambda x, y: y, "min": min, "max": max, "sum": lambda x, y: x + y}[counts]
    if op == "intersect":
        rows = {s: f(a[s], b[s]) for s in a if s in b}
    elif op == "subtract":
        rows = {s: a[s] for s in a if s not in b}
    else:
        rows = {s: f(a.get(s, 0), b.get(s, 0)) for s in set(a) | set(b)}
    return b"".join(b"%s\t%d\n" % (s, n) for s, n in sorted(rows.items())
                    if n >= max(1, lo) and (hi is None or n <= hi))


# ---------------------------------------------------------- key patterns

BASE = np.uint64(1 << 40)
MIXED = {"random", "extremes_both", "extremes_a", "extremes_b"}  # matched and unmatched rows of A both exist
GENERAL = ("interleaved", "below", "above", "random", "extremes_both", "extremes_a", "extremes_b")


def _random_pair(rng, na: int, nb: int):
    """About 40 % of the smaller table is shared."""
    m = int(0.4 * min(na, nb))
    total = na + nb - m
    pool = np.unique(rng.integers(1, (1 << 63) - 1, size=total + total // 8 + 16, dtype=np.int64).astype(np.uint64))
    pool = pool[rng.permutation(len(pool))[:total]]
    assert len(pool) == total
    ak = np.sort(pool[:na])                                   # pool[:m] shared, pool[m:na] A's own
    bk = np.sort(np.concatenate([pool[:m], pool[na:]]))       # pool[na:] B's own
    return ak, bk


def tables(pattern: str, na: int, nb: int, seed: int = 0):
    """(ak, bk): strictly ascending u64 keys of the pattern at these sizes."""
    rng = np.random.default_rng(1000 * seed + 31 * na + nb + len(pattern))
    ia, ib = np.arange(na, dtype=np.uint64), np.arange(nb, dtype=np.uint64)
    two = np.uint64(2)
    if pattern == "interleaved":  # disjoint
        return BASE + two * ia, BASE + two * ib + np.uint64(1)
    if pattern == "below":  # B wholly below A
        return BASE + np.uint64(nb + 10) + np.uint64(3) * ia, BASE + ib
    if pattern == "above":
        return BASE + np.uint64(3) * ia, BASE + np.uint64(3 * na + 10) + ib
    ak, bk = _random_pair(rng, na, nb)
    if pattern == "random":
        return ak, bk
    # keys 0 and 2^64 - 1 as the first and last row
    lo, hi = np.uint64(0), np.uint64(U64_MAX)
    if pattern in ("extremes_both", "extremes_a") and na >= 2:
        ak = ak.copy()
        ak[0], ak[-1] = lo, hi
    if pattern in ("extremes_both", "extremes_b") and nb >= 2:
        bk = bk.copy()
        bk[0], bk[-1] = lo, hi
    return ak, bk


def identical(n: int, seed: int = 0):
    ak, _ = _random_pair(np.random.default_rng(77 + n + seed), n, 0)
    return ak, ak.copy()


def shifted(n: int, seed: int = 0):
    """B = one smaller key, then A: every equal pair sits across a tile boundary somewhere."""
    ak, _ = identical(n, seed)
    return ak, np.concatenate([np.asarray([0], np.uint64), ak])


def packed(n_few: int, n_many: int, ends: bool):
    """A of n_few rows; B of n_many rows packed between A's two middle keys
    (ends: B's first and last row ARE those two keys)."""
    step = np.uint64(1 << 30)
    ak = BASE + step * np.arange(n_few, dtype=np.uint64)
    lo = ak[n_few // 2 - 1]
    if ends:
        bk = np.concatenate([[lo], lo + np.uint64(1) + np.arange(n_many - 2, dtype=np.uint64), [ak[n_few // 2]]])
    else:
        bk = lo + np.uint64(1) + np.arange(n_many, dtype=np.uint64)
    return ak, bk.astype(np.uint64)


def counts_for(rng, n: int, nbytes: int, small: bool = False) -> np.ndarray:
    """u32 counts 1..1000 (small: 1..6); u64 counts above 2^32."""
    c = rng.integers(1, 7 if small else 1001, n, dtype=np.int64).astype(np.uint64)
    if nbytes == 8:
        return c + (np.uint64(1 << 32) * rng.integers(1, 5, n, dtype=np.int64).astype(np.uint64))
    return c.astype(np.uint32)
