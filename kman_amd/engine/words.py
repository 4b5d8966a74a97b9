"""k-mers of any k as word planes (k > 32): extract, LSD sort, run-length rows."""

from __future__ import annotations

from ctypes import byref, c_int, c_uint64, c_void_p
from dataclasses import dataclass
from typing import Optional

from .. import _native as N
from .device import Device, DeviceBuffer, free_all
from .parsed import Parsed
from .kmers import MAX_K_WIDE, _check_k, count_kmers, flags_for


def nwords(k: int) -> int:
    """64-bit words per k-mer of the any-k path (words.hip): ceil(k / 32)."""
    return (k + 31) // 32


@dataclass
class Words:
    """k-mer keys of any k as W word planes (words.hip layout: word 0 the
    first k - 32 (W - 1) bases, then 32 bases per word, all MSB-first; word j
    of item i at words[j * stride + i]) + an optional u64 pos payload."""

    words: DeviceBuffer
    pos: Optional[DeviceBuffer]
    n: int
    k: int
    stride: int

    @property
    def W(self) -> int:
        return nwords(self.k)

    def plane(self, j: int) -> int:
        return self.words.ptr + 8 * j * self.stride

    def free(self) -> None:
        free_all(self.words, self.pos)


@dataclass
class WordsResult:
    """count / uniq rows of k > 32: keys as W word planes, row j's word q at
    words[q * stride + j] (stride: max(n, 1) of the rows as they were made; a
    filter_counts lowers n and leaves the planes where they are)."""

    words: DeviceBuffer
    vals: DeviceBuffer
    val_bytes: int
    n: int
    k: int
    mode: str
    stride: Optional[int] = None

    def __post_init__(self):
        if self.stride is None:
            self.stride = max(self.n, 1)

    @property
    def W(self) -> int:
        return nwords(self.k)

    def free(self) -> None:
        self.words.free()
        self.vals.free()


def extract_words(p: Parsed, k: int, rc: bool, want_pos: bool, canonical: bool = False) -> Words:
    """Keys (+ u64 pos) of the stream as word planes, in stream order
    (Sequence.yield_kmers, seq.py:285-328): kman_extract_wide's rolled
    LDS-staged kernel for k <= 64 (its (hi, lo) are planes 0 and 1),
    kman_extract_words beyond."""
    _check_k(k, wide=True)
    dev, L = p.dev, N.lib()
    n = count_kmers(p, k, rc, canonical)
    W = nwords(k)
    words = dev.alloc(8 * W * max(n, 1))
    pos = dev.alloc(8 * max(n, 1)) if want_pos else None
    w = Words(words, pos, n, k, max(n, 1))
    if n == 0:
        return w
    got = c_uint64(0)
    with dev.scratch() as s:
        s.own(w)
        if k <= MAX_K_WIDE:
            N.check(dev.ctx, L.kman_extract_wide(dev.ctx, c_void_p(p.codes.ptr), p.n_bases, k,
                                                 flags_for(rc, want_pos, canonical), c_void_p(w.plane(0)),
                                                 c_void_p(w.plane(1)), c_void_p(pos.ptr) if pos else None, 8, n,
                                                 byref(got)), "kman_extract_wide")
        else:
            N.check(dev.ctx, L.kman_extract_words(dev.ctx, c_void_p(p.codes.ptr), p.n_bases, k,
                                                  flags_for(rc, want_pos, canonical), c_void_p(words.ptr), w.stride,
                                                  c_void_p(pos.ptr) if pos else None, 8, n, byref(got)),
                    "kman_extract_words")
        s.keep(w)
    assert int(got.value) == n
    return w


def sort_words(w: Words, start: int = 0, per_batch: Optional[int] = None, dev: Optional[Device] = None) -> Words:
    """A stably sorted copy of word keys (+ pos): LSD over the planes, last
    word first, each a stable kman_sort of the gathered plane carrying the
    permutation (ties keep stream order, as the reference's Timsort,
    batch.py:156-168); per_batch: items in consecutive chunks of that many
    from stream index `start` sorted chunk by chunk (one Batch each) -- a
    final stable sort by the chunk tag (kman_batch_tags)."""
    dev, L = dev or w.words.dev, N.lib()
    n, W, k = w.n, w.W, w.k
    out = Words(dev.alloc(8 * W * max(n, 1)), dev.alloc(8 * max(n, 1)) if w.pos is not None else None, n, k,
                max(n, 1))
    if n == 0:
        return out
    with dev.scratch() as s:
        s.own(out)
        perm, key, alt_k, alt_p = [s.alloc(8 * n) for _ in range(4)]
        N.check(dev.ctx, L.kman_iota_u64(dev.ctx, c_void_p(perm.ptr), n), "iota")
        res = c_int(0)

        def stable(keys_, bits):
            nonlocal perm, alt_k, alt_p
            N.check(dev.ctx, L.kman_sort(dev.ctx, c_void_p(keys_.ptr), c_void_p(alt_k.ptr), c_void_p(perm.ptr),
                                         c_void_p(alt_p.ptr), 8, n, bits, None, byref(res)), "kman_sort")
            if res.value:  # (the sorted copy is in the alternates)
                perm, alt_p = alt_p, perm
                return alt_k, keys_
            return keys_, alt_k

        h = k - 32 * (W - 1)
        for j in reversed(range(W)):
            N.check(dev.ctx, L.kman_gather(dev.ctx, c_void_p(w.plane(j)), c_void_p(perm.ptr), n, c_void_p(key.ptr), 8),
                    "gather")
            key, alt_k = stable(key, 64 if j else 2 * h)
        if per_batch is not None:
            last = (start + n - 1) // per_batch
            N.check(dev.ctx, L.kman_batch_tags(dev.ctx, c_void_p(perm.ptr), n, start, per_batch, c_void_p(key.ptr)),
                    "kman_batch_tags")
            key, alt_k = stable(key, max(1, int(last).bit_length()))
        for j in range(W):
            N.check(dev.ctx, L.kman_gather(dev.ctx, c_void_p(w.plane(j)), c_void_p(perm.ptr), n,
                                           c_void_p(out.plane(j)), 8), "gather")
        if w.pos is not None:
            N.check(dev.ctx, L.kman_gather(dev.ctx, c_void_p(w.pos.ptr), c_void_p(perm.ptr), n, c_void_p(out.pos.ptr),
                                           8), "gather")
        return s.keep(out)


def rle_words(w: Words, mode: str) -> WordsResult:
    """Run-length rows of sorted word keys (Crawler.do_batch + the count /
    uniq writers, join.py:95-130, 244-285)."""
    dev, L = w.words.dev, N.lib()
    n, W = w.n, w.W
    uniq = mode == "uniq"
    vb = 8 if uniq else (4 if n <= 0xFFFFFFFF else 8)
    out = c_uint64(0)
    with dev.scratch() as s:
        ow = s.alloc(8 * W * max(n, 1))
        ov = s.alloc(vb * max(n, 1))
        N.check(dev.ctx, L.kman_rle_words(dev.ctx, N.KMAN_FINISH_UNIQ if uniq else N.KMAN_FINISH_COUNT,
                                          c_void_p(w.words.ptr), W, w.stride, c_void_p(w.pos.ptr) if uniq else None,
                                          8, n, c_void_p(ow.ptr), max(n, 1), c_void_p(ov.ptr), vb, byref(out)),
                "kman_rle_words")
        s.keep(ow), s.keep(ov)
    # (planes keep the input's stride n: row j's word q at ow[q * n + j])
    return WordsResult(ow, ov, vb, int(out.value), w.k, mode, stride=max(n, 1))


def words_groups(p: Parsed, k: int, rc: bool, mode: str, canonical: bool = False) -> Optional[WordsResult]:
    """k > 32 (seq.py:285-328 has no k limit): the keys as word planes
    (extract_words), an LSD sort over the planes (sort_words,
    batch.py:156-168), kman_rle_words (join.py:95-130, 244-285).  None when
    the stream has no k-mers."""
    w = extract_words(p, k, rc, mode == "uniq", canonical)
    try:
        if w.n == 0:
            return None
        sw = sort_words(w)
    finally:
        w.free()
    try:
        return rle_words(sw, mode)
    finally:
        sw.free()


wide_groups = words_groups  # (the word-pair name of round 2: k in 33..64 is W = 2)
