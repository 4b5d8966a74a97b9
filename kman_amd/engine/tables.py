"""Count tables: the abundance filter, set operations, the prefix index and the lookup preamble."""

from __future__ import annotations

from ctypes import byref, c_uint64, c_void_p
from typing import Optional, Tuple

import numpy as np

from .. import _native as N
from .device import Device, DeviceBuffer, Scratch
from .kmers import CountResult, MAX_K
from .words import WordsResult


def check_count_range(min_count=1, max_count=None) -> Tuple[int, Optional[int]]:
    """The abundance range of filter_counts, checked: integers >= 1,
    `max_count` None (no upper bound) or >= `min_count`."""
    for name, v in (("min_count", min_count), ("max_count", max_count)):
        if v is None and name == "max_count":
            continue
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < 1:
            raise AssertionError("%s must be an integer >= 1, got %r" % (name, v))
    if max_count is not None and min_count > max_count:
        raise AssertionError("min_count %d is greater than max_count %d" % (min_count, max_count))
    return int(min_count), None if max_count is None else int(max_count)


def _count_rows(r):
    """(key planes ptr, W, stride, counts ptr, count bytes) of a count result."""
    if isinstance(r, WordsResult):
        if r.mode != "count":
            raise ValueError("filter_counts takes count rows, not uniq rows")
        return r.words.ptr, r.W, r.stride, r.vals.ptr, r.val_bytes
    if not isinstance(r, CountResult):
        raise ValueError("filter_counts takes a CountResult or a count-mode WordsResult")
    return r.ukeys.ptr, 1, max(r.n, 1), r.counts.ptr, r.count_bytes


def _filter_call(dev: Device, r, lo: int, hi: int, okeys, ocounts) -> int:
    kp, W, stride, cp, cb = _count_rows(r)
    out = c_uint64(0)
    N.check(dev.ctx, N.lib().kman_filter_counts(dev.ctx, c_void_p(kp), W, stride, c_void_p(cp), cb, r.n, lo, hi,
                                                c_void_p(okeys), c_void_p(ocounts), byref(out)), "kman_filter_counts")
    return int(out.value)


_U64_MAX = (1 << 64) - 1


def filter_counts(dev: Device, r, min_count: int = 1, max_count: Optional[int] = None):
    """Keep the rows of a count result (CountResult, or a count-mode
    WordsResult) whose count is in [min_count, max_count], in their order, in
    place on the device (kman_filter_counts): r.n becomes the rows kept, the
    buffers (and a WordsResult's stride) stay.  Returns r.  The identity
    range (min_count <= 1, no max_count) launches nothing."""
    if r is None or (min_count <= 1 and max_count is None):
        return r
    lo, hi = check_count_range(max(1, min_count), max_count)
    kp, _, _, cp, _ = _count_rows(r)
    r.n = _filter_call(dev, r, lo, _U64_MAX if hi is None else hi, kp, cp)
    return r


def filtered_copy(dev: Device, r: CountResult, min_count: int = 1, max_count: Optional[int] = None) -> CountResult:
    """filter_counts out of place: the kept rows of a CountResult in fresh
    buffers sized by a counting call first; r and its buffers are left as
    they are (rows that are read again, such as a pipeline's)."""
    lo, hi = check_count_range(min_count, max_count)
    hi = _U64_MAX if hi is None else hi
    n = _filter_call(dev, r, lo, hi, None, None)
    with dev.scratch() as s:
        ok_ = s.alloc(8 * max(n, 1))
        oc_ = s.alloc(r.count_bytes * max(n, 1))
        if n:
            got = _filter_call(dev, r, lo, hi, ok_.ptr, oc_.ptr)
            assert got == n
        return CountResult(s.keep(ok_), s.keep(oc_), r.count_bytes, n, r.k)


MATCH_OPS = {
    "right": N.KMAN_MATCH_RIGHT, "left": N.KMAN_MATCH_LEFT, "min": N.KMAN_MATCH_MIN, "max": N.KMAN_MATCH_MAX,
    "sum": N.KMAN_MATCH_SUM, "absent": N.KMAN_MATCH_ABSENT, "any_sum": N.KMAN_MATCH_ANY_SUM,
    "any_max": N.KMAN_MATCH_ANY_MAX,
}
SET_OPS = {  # op -> the `counts` choices it takes, the default first
    "intersect": ("left", "right", "min", "max", "sum"),
    "subtract": ("left",),
    "union": ("sum", "max"),
}


def check_set_op(op: str, counts: Optional[str] = None) -> str:
    """The `counts` choice of set_op(op), checked (AssertionError); None: the
    op's default."""
    if op not in SET_OPS:
        raise AssertionError("op must be one of %s, got %r" % (", ".join(SET_OPS), op))
    if counts is None:
        return SET_OPS[op][0]
    if counts not in SET_OPS[op]:
        raise AssertionError("--counts %s: --op %s takes %s" % (counts, op, " | ".join(SET_OPS[op])))
    return counts


def empty_count(dev: Device, k: int) -> CountResult:
    """The count table of an input without k-mers: the empty set."""
    return CountResult(dev.alloc(8), dev.alloc(4), 4, 0, k)


def _match_bytes(a: CountResult, b: CountResult) -> int:
    return 8 if 8 in (a.count_bytes, b.count_bytes) else 4


def match_counts(dev: Device, a: CountResult, b: CountResult, op: str = "right") -> DeviceBuffer:
    """kman_match_counts: one value per row of `a` from the row of `b` with
    the same key (MATCH_OPS; include/kman.h), as a fresh device vector of
    a.n values, 4 bytes wide unless either table's counts are 8.  `a` and `b`
    are key-sorted distinct count rows of one k (join_groups(.., "count"))."""
    if op not in MATCH_OPS:
        raise AssertionError("match op must be one of %s, got %r" % (", ".join(MATCH_OPS), op))
    if a.k != b.k:
        raise AssertionError("the two tables hold k-mers of different k: %d and %d" % (a.k, b.k))
    ob = _match_bytes(a, b)
    with dev.scratch() as s:
        out = s.alloc(ob * max(a.n, 1))
        N.check(dev.ctx, N.lib().kman_match_counts(
            dev.ctx, c_void_p(a.ukeys.ptr), c_void_p(a.counts.ptr), a.count_bytes, a.n, c_void_p(b.ukeys.ptr),
            c_void_p(b.counts.ptr), b.count_bytes, b.n, MATCH_OPS[op], c_void_p(out.ptr), ob), "kman_match_counts")
        return s.keep(out)


def _matched_rows(dev: Device, a: CountResult, b: CountResult, op: str, lo: int = 1,
                  hi: Optional[int] = None) -> CountResult:
    """The rows (key of a, match_counts(a, b, op)) whose value is in [lo, hi],
    in fresh buffers: the match vector, then one out-of-place filter over a's
    keys and that vector (rows whose value is 0 are dropped: lo >= 1)."""
    with dev.scratch() as s:
        v = s.own(match_counts(dev, a, b, op))
        return filtered_copy(dev, CountResult(a.ukeys, v, _match_bytes(a, b), a.n, a.k), lo, hi)


def set_op(dev: Device, a: CountResult, b: CountResult, op: str, counts: Optional[str] = None, min_count: int = 1,
           max_count: Optional[int] = None) -> CountResult:
    """Set operations on two count tables of one k, on the device; a fresh
    CountResult (key-sorted, distinct), `a` and `b` left as they are.
      intersect  the rows of a whose key is in b; counts: left (default, a's) |
                 right (b's) | min | max | sum
      subtract   the rows of a whose key is not in b, with a's counts
      union      every key of either; counts: sum (default) | max
    Only rows whose resulting count is in [max(1, min_count), max_count] are
    kept.  intersect / subtract: kman_match_counts + one out-of-place
    kman_filter_counts (the range costs no pass of its own); union: a's rows
    with ANY_SUM / ANY_MAX, b's rows absent from a, one 2-run kman_merge_runs,
    then the range.  No row is downloaded."""
    counts = check_set_op(op, counts)
    if a.k != b.k:
        raise AssertionError("the two tables hold k-mers of different k: %d and %d" % (a.k, b.k))
    lo, hi = check_count_range(max(1, min_count) if isinstance(min_count, (int, np.integer)) else min_count,
                               max_count)
    if op == "intersect":
        return _matched_rows(dev, a, b, counts, lo, hi)
    if op == "subtract":
        return _matched_rows(dev, a, b, "absent", lo, hi)
    vb = _match_bytes(a, b)
    with dev.scratch() as s:
        va = s.own(match_counts(dev, a, b, "any_" + counts))
        only_b = _matched_rows(dev, b, a, "absent")
        s.own(only_b.ukeys), s.own(only_b.counts)
        n = a.n + only_b.n
        ok_ = s.alloc(8 * max(n, 1))
        oc_ = s.alloc(vb * max(n, 1))
        runs = (N.Run * 2)(N.Run(a.ukeys.ptr, va.ptr, a.n), N.Run(only_b.ukeys.ptr, only_b.counts.ptr, only_b.n))
        N.check(dev.ctx, N.lib().kman_merge_runs(dev.ctx, runs, 2, vb, c_void_p(ok_.ptr), c_void_p(oc_.ptr), None,
                                                 None), "kman_merge_runs")
        r = CountResult(ok_, oc_, vb, n, a.k)
        filter_counts(dev, r, lo, hi)
        s.keep(ok_), s.keep(oc_)  # (the result's now)
        return r


def default_index_bits(n: int, k: int) -> int:
    """table_index's default width: about 8 rows per bucket on spread keys."""
    return min(2 * k, N.KMAN_SCREEN_MAX_INDEX_BITS, max(1, (max(int(n), 2) - 1).bit_length() - 3))


def _check_index_bits(index_bits: int, k: int) -> int:
    top = min(2 * k, N.KMAN_SCREEN_MAX_INDEX_BITS)
    if isinstance(index_bits, bool) or not isinstance(index_bits, (int, np.integer)) or not 1 <= index_bits <= top:
        raise AssertionError("index_bits must be an integer in [1, %d] for k = %d, got %r" % (top, k, index_bits))
    return int(index_bits)


def _check_key_k(k: int, what: str) -> None:
    """A table lookup takes keys of one word; `what`: the caller's name in the message."""
    if k > MAX_K:
        raise AssertionError("%s takes k <= %d (one 64-bit key per k-mer), got %d" % (what, MAX_K, k))


def _index_bits(table: CountResult, index_bits: Optional[int]) -> int:
    """The width of a table's index: the caller's, checked, or the default."""
    return default_index_bits(table.n, table.k) if index_bits is None else _check_index_bits(index_bits, table.k)


def _index(scope: Scratch, table: CountResult, index: Optional[DeviceBuffer], bits: int) -> DeviceBuffer:
    """The caller's index, or a table_index built here and owned by `scope`."""
    return scope.own(table_index(scope.dev, table, bits)) if index is None else index


def table_index(dev: Device, table: CountResult, index_bits: Optional[int] = None) -> DeviceBuffer:
    """kman_table_index: the prefix index of a key-sorted distinct count table
    (join_groups(.., "count")), 2^index_bits + 1 u64 words in a fresh device
    buffer: word p = the rows whose top index_bits key bits are < p.
    index_bits None: min(2k, 24, max(1, ceil(log2(max(n, 2))) - 3)), about 8
    rows per bucket on spread keys -- a choice nobody has measured against
    wider or narrower indexes."""
    _check_key_k(table.k, "a table index")
    bits = _index_bits(table, index_bits)
    with dev.scratch() as s:
        idx = s.alloc(8 * ((1 << bits) + 1))
        N.check(dev.ctx, N.lib().kman_table_index(dev.ctx, c_void_p(table.ukeys.ptr), table.n, table.k, bits,
                                                  c_void_p(idx.ptr)), "kman_table_index")
        return s.keep(idx)
