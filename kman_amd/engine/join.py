"""count / uniq of a whole stream by the path that takes it: region, key rounds, RangedJoin, general."""

from __future__ import annotations

from ctypes import byref, c_uint64, c_void_p
from typing import List, Optional, Tuple

import numpy as np

from .. import _native as N
from .device import DeviceBuffer, mem_info
from .parsed import Parsed
from .kmers import (
    CountResult, Kmers, MAX_K, UniqResult, _check_k, _finish, _sort_prefix, extract_sorted, flags_for, groups,
    rle_count, rle_uniq, split_bits,
)
from .words import WordsResult, words_groups


def _prefix_hist_into(p: Parsed, k: int, rc: bool, h: DeviceBuffer) -> Tuple[np.ndarray, int]:
    n = c_uint64(0)
    N.check(p.dev.ctx, N.lib().kman_kmer_prefix_hist(p.dev.ctx, c_void_p(p.codes.ptr), p.n_bases, k,
                                                      N.KMAN_RC if rc else 0, c_void_p(h.ptr), byref(n)),
            "kman_kmer_prefix_hist")
    bins = 256 if 2 * k >= 8 else 1 << (2 * k)
    return p.dev.download(h, bins, np.uint64), int(n.value)


def prefix_hist(p: Parsed, k: int, rc: bool) -> Tuple[np.ndarray, int]:
    """Histogram of the top 8 key bits of the stream (kman_kmer_prefix_hist):
    4^k bins when 2k < 8.  Returns (hist, n_kmers)."""
    _check_k(k)
    with p.dev.scratch() as s:
        return _prefix_hist_into(p, k, rc, s.alloc(8 * 256))


def key_ranges(hist: np.ndarray, k: int, max_keys: int, count=None) -> List[Tuple[int, int, int]]:
    """Consecutive top-8-bit prefixes grouped into key ranges of at most
    max_keys k-mers: [(key_lo, key_hi, n)] in key order, empty ranges dropped.
    The batches of a multi-batch join (join.py:63-130) cut by key instead of
    by stream position: their n-way merge is then their concatenation.  A
    prefix holding more than max_keys k-mers (repeats, poly-A) is bisected
    by key with count(lo, hi) -> k-mers in [lo, hi] until its pieces fit;
    only one key value repeated more than max_keys times cannot be cut."""
    shift = max(0, 2 * k - 8)
    out, lo, acc = [], 0, 0

    def split(a, b, c):
        if c <= max_keys:
            return [(a, b, c)] if c else []
        if a == b or count is None:
            raise MemoryError("%d k-mers in key range [%x, %x]: more than a batch of %d" % (c, a, b, max_keys))
        m = (a + b) // 2
        c0 = count(a, m)
        return split(a, m, c0) + split(m + 1, b, c - c0)

    for b, c in enumerate(hist.tolist()):
        if c > max_keys:
            if acc:
                out.append((lo << shift, (b << shift) - 1, acc))
            out.extend(split(b << shift, ((b + 1) << shift) - 1, c))
            lo, acc = b + 1, 0
            continue
        if acc and acc + c > max_keys:
            out.append((lo << shift, (b << shift) - 1, acc))
            lo, acc = b, 0
        acc += c
    if acc:
        out.append((lo << shift, (len(hist) << shift) - 1, acc))
    return out


class _At:
    """A device pointer inside a buffer (an output slice) for _finish."""

    def __init__(self, buf: DeviceBuffer, offset: int):
        self.ptr = buf.ptr + int(offset)


class RangedJoin:
    """Multi-batch device join (BASELINE config 3): count / uniq of a stream
    whose k-mers do not fit the device at once.  The stream is cut into key
    ranges of at most max_keys k-mers (prefix_hist + key_ranges); each range
    is extracted from the resident codes (kman_extract_range, stream order),
    prefix-sorted (kman_sort_range) and finished in LDS (kman_finish), its
    output appended to the global output, which is therefore in key order.
    Same results as groups() / extract_sorted + rle_* (join.py:95-130,
    244-285 over batch.py:156-168).  Every buffer is allocated here, once:
    ``step()`` re-plans (prefix histogram) and runs the batches."""

    def __init__(self, p: Parsed, k: int, rc: bool, mode: str, max_keys: Optional[int] = None):
        _check_k(k)
        self.p, self.k, self.rc, self.mode = p, k, rc, mode
        dev = self.dev = p.dev
        self.want_pos = mode == "uniq"
        self._bufs = []
        self.phist = self._alloc(8 * 256)
        hist, n = _prefix_hist_into(p, k, rc, self.phist)
        self.n_kmers = n
        self.pos_bytes = 4 if 2 * p.n_bases <= 0xFFFFFFFF else 8
        self.vb = self.pos_bytes if self.want_pos else (4 if n <= 0xFFFFFFFF else 8)
        per_key = 16 + (2 * self.pos_bytes if self.want_pos else 0)
        if max_keys is None:
            free, _ = mem_info(dev)
            max_keys = max(1 << 20, (int(free * 0.85) - (8 + self.vb) * n) // per_key)
        self.max_keys = int(max_keys)
        self.ranges = key_ranges(hist, k, self.max_keys, self._count_range)
        self.cap = max([r[2] for r in self.ranges] + [1])
        self.okeys = self._alloc(8 * max(n, 1))
        self.ovals = self._alloc(self.vb * max(n, 1))
        self.keys, self.alt = self._alloc(8 * self.cap), self._alloc(8 * self.cap)
        self.pos = self._alloc(self.pos_bytes * self.cap) if self.want_pos else None
        self.pos_alt = self._alloc(self.pos_bytes * self.cap) if self.want_pos else None
        self.hbuf = self._alloc(8 * 256 * 8)
        self.n_out = 0

    def _count_range(self, lo: int, hi: int) -> int:
        """k-mers with keys in [lo, hi] (kman_extract_range with no capacity:
        counted, nothing written)."""
        got = c_uint64(0)
        rc = N.lib().kman_extract_range(self.dev.ctx, c_void_p(self.p.codes.ptr), self.p.n_bases, self.k,
                                        flags_for(self.rc, False), lo, hi, None, None, 4, 0, None, byref(got))
        if rc not in (N.KMAN_OK, N.KMAN_ECAP):
            N.check(self.dev.ctx, rc, "kman_extract_range")
        return int(got.value)

    def _alloc(self, nbytes: int) -> DeviceBuffer:
        try:
            b = self.dev.alloc(nbytes)
        except BaseException:
            self.free()
            raise
        self._bufs.append(b)
        return b

    def step(self) -> int:
        """One whole join: plan the key ranges, then extract + sort + finish
        each range into the output.  Returns the number of k-mers joined."""
        dev, L, k, p = self.dev, N.lib(), self.k, self.p
        hist, n = _prefix_hist_into(p, k, self.rc, self.phist)
        ranges = self.ranges
        if n != self.n_kmers:
            raise RuntimeError("the stream changed under a planned RangedJoin")
        flags = flags_for(self.rc, self.want_pos)
        fmode = N.KMAN_FINISH_UNIQ if self.want_pos else N.KMAN_FINISH_COUNT
        shift = max(0, 2 * k - 8)
        vb, pb = self.vb, self.pos_bytes
        total = 0
        for lo_key, hi_key, nr in ranges:
            # the range's keys fill (hi - lo + 1) of the len(hist) prefixes:
            # segment bits as for a stream that dense over the whole key space
            lo = split_bits(nr * (1 << (2 * k)) // (hi_key - lo_key + 1), 2 * k)
            dev.memset(self.hbuf, 0, 8 * 256 * 8)
            got = c_uint64(0)
            N.check(dev.ctx, L.kman_extract_range(dev.ctx, c_void_p(p.codes.ptr), p.n_bases, k,
                                                  flags | N.KMAN_HIST_LO(lo), lo_key, hi_key,
                                                  c_void_p(self.keys.ptr),
                                                  c_void_p(self.pos.ptr if self.pos else None), pb, self.cap,
                                                  c_void_p(self.hbuf.ptr), byref(got)), "kman_extract_range")
            if int(got.value) != nr:
                raise RuntimeError("key range [%x, %x]: %d k-mers extracted, histogram said %d"
                                   % (lo_key, hi_key, got.value, nr))
            km = Kmers(self.keys, self.alt, self.pos, self.pos_alt, pb if self.want_pos else 0, nr, k, self.hbuf,
                       lo_bit=lo, hist_valid=True)
            _sort_prefix(km, dev, 2 * k)
            total += _finish(km, dev, 2 * k, fmode, _At(self.okeys, 8 * total), _At(self.ovals, vb * total), vb)
            self.keys, self.alt, self.pos, self.pos_alt = km.keys, km.alt, km.pos, km.pos_alt
        self.n_out = total
        return n

    def result(self):
        """The output (CountResult / UniqResult); its buffers now belong to
        the caller."""
        r = (UniqResult if self.want_pos else CountResult)(self.okeys, self.ovals, self.vb, self.n_out, self.k)
        self._bufs = [b for b in self._bufs if b is not self.okeys and b is not self.ovals]
        return r

    def free(self) -> None:
        for b in self._bufs:
            b.free()
        self._bufs = []


def ranged_groups(p: Parsed, k: int, rc: bool, mode: str, max_keys: Optional[int] = None):
    """RangedJoin in one call: the CountResult / UniqResult of the stream."""
    j = RangedJoin(p, k, rc, mode, max_keys)
    try:
        j.step()
        return j.result()
    finally:
        j.free()


def _fits(p: Parsed, k: int, rc: bool, mode: str) -> bool:
    """Does the single-batch general path (extract_sorted + rle_*) fit the
    free HBM?  If not, the multi-batch join (ranged_groups) takes the input."""
    n = p.n_bases * (2 if rc else 1)
    pb = 4 if 2 * p.n_bases <= 0xFFFFFFFF else 8
    need = n * (16 + 8 + (3 * pb if mode == "uniq" else (4 if n <= 0xFFFFFFFF else 8)))
    return need <= 0.85 * mem_info(p.dev)[0]


def count_groups(p: Parsed, k: int, rc: bool = False, canonical: bool = False, ordered: bool = True) -> CountResult:
    """(key, count) per distinct k-mer on the device: the region path, else
    the prefix-split path (None only when there are no k-mers).
    ordered=False: the rows may come in any order (a spectrum needs only
    the multiset; the key rounds then skip merging a redone key range).
    k > 32: a WordsResult (word keys, its counts in .vals)."""
    if k > MAX_K:
        return words_groups(p, k, rc, "count", canonical)
    # a spectrum (ordered=False) of canonical keys counts mixed keys
    # (KMAN_MIXED): the same counts, uniform buckets for the region passes
    mixed = canonical and not ordered
    r = groups(p, k, rc, "count", canonical, mixed)
    if r is not None:
        return r
    if p.n_bases:
        from .. import dist

        r = dist.local_groups(p, k, rc, "count", canonical, ordered=ordered)
        if r is not None:
            return r
    km = extract_sorted(p, k, rc, want_pos=False, canonical=canonical)
    try:
        if km.n == 0:
            return None
        return rle_count(km, p.dev)
    finally:
        km.free()


def join_groups(p: Parsed, k: int, rc: bool, mode: str, max_keys: Optional[int] = None, canonical: bool = False):
    """The count / uniq result of the whole stream of p on the device, by the
    fastest path that takes it: the region path (kman_groups); the multi-batch
    join (RangedJoin) when the single-batch general path does not fit the
    free HBM or max_keys asks for it; else the general path (extract_sorted +
    rle_*); k > 32: the word-pair path (wide_groups).  None when the stream
    has no k-mers.  canonical: the rows of min(k-mer, reverse complement)
    (count only; `rc` is then moot, both strands fold into one key); a
    sub-path that cannot take canonical keys raises NotImplementedError."""
    if canonical and mode == "uniq":
        raise ValueError("canonical k-mers are counted (config 5), not uniq'd")
    if k > MAX_K:
        return words_groups(p, k, rc, mode, canonical)
    r = groups(p, k, rc, mode, canonical) if max_keys is None else None
    if r is None and max_keys is None and p.n_bases:
        # outside kman_groups (too many k-mers for its regions, -r on large
        # inputs, skewed keys): the key rounds of the multi-GPU path on one GPU
        from .. import dist

        r = dist.local_groups(p, k, rc, mode, canonical)
    if r is None and (max_keys is not None or not _fits(p, k, rc and not canonical, mode)):
        if canonical:
            # (RangedJoin cuts the stream by forward-key ranges: kman_extract_range has no canonical keys)
            raise NotImplementedError("canonical k-mers through the multi-batch join (RangedJoin)")
        r = ranged_groups(p, k, rc, mode, max_keys)
    if r is None:
        km = extract_sorted(p, k, rc, want_pos=mode == "uniq", canonical=canonical)
        try:
            if km.n == 0:
                return None
            r = rle_count(km, p.dev) if mode == "count" else rle_uniq(km, p.dev)
        finally:
            km.free()
    return r


def free_result(r) -> None:
    if r is None:
        return
    if isinstance(r, WordsResult):
        bs = (r.words, r.vals)
    else:
        bs = (r.ukeys, r.counts) if isinstance(r, CountResult) else (r.keys, r.pos)
    for b in bs:
        b.free()
