"""k-mers of k <= 32 as one 64-bit key each: extract, sort, run-length rows, the region path."""

from __future__ import annotations

import ctypes
from ctypes import byref, c_int, c_uint64, c_void_p
from dataclasses import dataclass
from typing import Optional

from .. import _native as N
from .. import phases
from .device import Device, DeviceBuffer, free_all
from .parsed import Parsed


MAX_K = 32       # 2-bit keys in one u64 (the region / prefix-split paths)
MAX_K_WIDE = 64  # k <= 64: kman_extract_wide rolls the two words of a key; beyond, kman_extract_words


@dataclass
class Kmers:
    """k-mer keys (+ pos payload) in the reference's stream order."""

    keys: DeviceBuffer
    alt: DeviceBuffer
    pos: Optional[DeviceBuffer]
    pos_alt: Optional[DeviceBuffer]
    pos_bytes: int
    n: int
    k: int
    hist: DeviceBuffer
    sorted: bool = False
    # histogram plan of kman_extract: bits [lo_bit, 2k) (kman_split_bits);
    # hist_valid False = no usable histogram (sort computes its own)
    lo_bit: int = 0
    hist_valid: bool = False
    prefix_sorted: bool = False  # keys stably sorted by bits [lo_bit, 2k) (kman_extract_sorted)

    def free(self) -> None:
        free_all(self.keys, self.alt, self.pos, self.pos_alt, self.hist)


def flags_for(rc: bool, want_pos: bool, canonical: bool = False, mixed: bool = False) -> int:
    """kman_extract flags; mixed (with canonical): the keys through the
    bijection of KMAN_MIXED -- spectra only, the keys are not printed."""
    return ((N.KMAN_RC if rc else 0) | (N.KMAN_WANT_POS if want_pos else 0) | (N.KMAN_CANONICAL if canonical else 0)
            | (N.KMAN_MIXED if canonical and mixed else 0))


def count_kmers(p: Parsed, k: int, rc: bool, canonical: bool = False) -> int:
    _check_k(k, wide=True)
    out = c_uint64(0)
    if k > MAX_K_WIDE:
        N.check(p.dev.ctx, N.lib().kman_extract_words(p.dev.ctx, c_void_p(p.codes.ptr), p.n_bases, k,
                                                      flags_for(rc, False, canonical), None, 0, None, 0, 0,
                                                      byref(out)), "kman_extract_words")
        return int(out.value)
    if k > MAX_K:
        N.check(p.dev.ctx, N.lib().kman_extract_wide(p.dev.ctx, c_void_p(p.codes.ptr), p.n_bases, k,
                                                     flags_for(rc, False, canonical), None, None, None, 0, 0,
                                                     byref(out)), "kman_extract_wide")
        return int(out.value)
    N.check(p.dev.ctx, N.lib().kman_count_kmers(p.dev.ctx, c_void_p(p.codes.ptr), p.n_bases, k,
                                                 flags_for(rc, False, canonical), byref(out)), "kman_count_kmers")
    return int(out.value)


def _check_k(k: int, wide: bool = False) -> None:
    """batcher.py:477-478 (k <= 1 raises AssertionError); a path that packs a
    k-mer in one 64-bit key (region / prefix-split / multi-GPU) takes
    k <= 32, the word-key path (wide) every k."""
    if k <= 1:
        raise AssertionError("k must be >= 1, got %d instead." % k)
    if not wide and k > MAX_K:
        raise NotImplementedError("k=%d: this path packs k-mers in one 64-bit key (k <= %d); the word-key path "
                                  "takes larger k" % (k, MAX_K))


def extract(p: Parsed, k: int, rc: bool, want_pos: bool, canonical: bool = False) -> Kmers:
    """kman_extract: keys (+ pos) in stream order, plus the radix histograms."""
    _check_k(k)
    dev = p.dev
    L = N.lib()
    bound = p.n_bases * (2 if rc and not canonical else 1)
    n = max(bound, 1)
    pos_bytes = 4 if 2 * p.n_bases <= 0xFFFFFFFF else 8
    keys = dev.alloc(8 * n)
    alt = dev.alloc(8 * n)
    pos = dev.alloc(pos_bytes * n) if want_pos else None
    pos_alt = dev.alloc(pos_bytes * n) if want_pos else None
    hist = dev.alloc(8 * 256 * 8)
    dev.memset(hist, 0, 8 * 256 * 8)
    out = c_uint64(0)
    lo = split_bits(bound, 2 * k)
    rc_ = L.kman_extract(dev.ctx, c_void_p(p.codes.ptr), p.n_bases, k,
                         flags_for(rc, want_pos, canonical) | N.KMAN_HIST_LO(lo),
                         c_void_p(keys.ptr), c_void_p(pos.ptr if pos else None), pos_bytes, bound,
                         c_void_p(hist.ptr), byref(out))
    N.check(dev.ctx, rc_, "kman_extract")
    return Kmers(keys, alt, pos, pos_alt, pos_bytes if want_pos else 0, int(out.value), k, hist, lo_bit=lo,
                 hist_valid=True)


def extract_sorted(p: Parsed, k: int, rc: bool, want_pos: bool, canonical: bool = False) -> Kmers:
    """kman_extract_sorted: the k-mers already stably sorted by their prefix
    bits [lo, 2k) (first prefix pass fused into the extraction)."""
    _check_k(k)
    dev = p.dev
    L = N.lib()
    bound = p.n_bases * (2 if rc and not canonical else 1)
    n = max(bound, 1)
    pos_bytes = 4 if 2 * p.n_bases <= 0xFFFFFFFF else 8
    keys, alt = dev.alloc(8 * n), dev.alloc(8 * n)
    pos = dev.alloc(pos_bytes * n) if want_pos else None
    pos_alt = dev.alloc(pos_bytes * n) if want_pos else None
    lo = split_bits(bound, 2 * k)
    out, res = c_uint64(0), c_int(0)
    N.check(dev.ctx, L.kman_extract_sorted(dev.ctx, c_void_p(p.codes.ptr), p.n_bases, k,
                                           flags_for(rc, want_pos, canonical), lo,
                                           c_void_p(keys.ptr), c_void_p(alt.ptr),
                                           c_void_p(pos.ptr if pos else None), c_void_p(pos_alt.ptr if pos else None),
                                           pos_bytes, bound, byref(out), byref(res)), "kman_extract_sorted")
    if res.value:
        keys, alt = alt, keys
        pos, pos_alt = pos_alt, pos
    return Kmers(keys, alt, pos, pos_alt, pos_bytes if want_pos else 0, int(out.value), k, dev.alloc(8), lo_bit=lo,
                 prefix_sorted=True)


def split_bits(n: int, key_bits: int) -> int:
    """kman_split_bits: low bit of the prefix the global passes sort by."""
    lo = ctypes.c_uint32(0)
    if N.lib().kman_split_bits(max(int(n), 0), key_bits, byref(lo)) != N.KMAN_OK:
        raise ValueError("bad key_bits %d" % key_bits)
    return int(lo.value)


def _sort_prefix(km: Kmers, dev: Device, key_bits: int) -> None:
    """kman_sort_range over bits [km.lo_bit, key_bits): a stable sort by the
    prefix; km.keys / km.pos then hold the prefix-sorted data."""
    if km.prefix_sorted:
        return
    res = c_int(0)
    hist = c_void_p(km.hist.ptr) if km.hist_valid and km.hist is not None else c_void_p(None)
    rc = N.lib().kman_sort_range(dev.ctx, c_void_p(km.keys.ptr), c_void_p(km.alt.ptr),
                                 c_void_p(km.pos.ptr if km.pos else None),
                                 c_void_p(km.pos_alt.ptr if km.pos_alt else None), km.pos_bytes, km.n, km.lo_bit,
                                 key_bits, hist, byref(res))
    N.check(dev.ctx, rc, "kman_sort_range")
    if res.value:
        km.keys, km.alt = km.alt, km.keys
        km.pos, km.pos_alt = km.pos_alt, km.pos
    km.prefix_sorted = True


def _finish(km: Kmers, dev: Device, key_bits: int, mode: int, okeys=None, ovals=None, ob: int = 0) -> int:
    out = c_uint64(0)
    N.check(dev.ctx, N.lib().kman_finish(dev.ctx, c_void_p(km.keys.ptr), c_void_p(km.alt.ptr),
                                         c_void_p(km.pos.ptr if km.pos else None),
                                         c_void_p(km.pos_alt.ptr if km.pos_alt else None), km.pos_bytes, km.n,
                                         key_bits, km.lo_bit, mode, c_void_p(okeys.ptr if okeys else None),
                                         c_void_p(ovals.ptr if ovals else None), ob, byref(out)), "kman_finish")
    return int(out.value)


def sort(km: Kmers, dev: Device) -> None:
    """Stable sort of km.keys (+ km.pos) by key, Batch.sorted (batch.py:156-168):
    kman_sort_range over the prefix bits, then kman_finish(SORT) in LDS."""
    if km.sorted:
        return
    if km.n > 1:
        _sort_prefix(km, dev, 2 * km.k)
        _finish(km, dev, 2 * km.k, N.KMAN_FINISH_SORT)
    km.sorted = True


@dataclass
class CountResult:
    ukeys: DeviceBuffer
    counts: DeviceBuffer
    count_bytes: int
    n: int
    k: int


def rle_count(km: Kmers, dev: Device) -> CountResult:
    """(key, group size) per distinct key.  Sorted input: kman_rle_count;
    unsorted: the prefix sort + kman_finish(COUNT) (km is consumed)."""
    cb = 4 if km.n <= 0xFFFFFFFF else 8
    ukeys = dev.alloc(8 * max(km.n, 1))
    counts = dev.alloc(cb * max(km.n, 1))
    if not km.sorted:
        _sort_prefix(km, dev, 2 * km.k)
        n = _finish(km, dev, 2 * km.k, N.KMAN_FINISH_COUNT, ukeys, counts, cb)
        return CountResult(ukeys, counts, cb, n, km.k)
    out = c_uint64(0)
    N.check(dev.ctx, N.lib().kman_rle_count(dev.ctx, c_void_p(km.keys.ptr), km.n, c_void_p(ukeys.ptr),
                                             c_void_p(counts.ptr), cb, byref(out)), "kman_rle_count")
    return CountResult(ukeys, counts, cb, int(out.value), km.k)


@dataclass
class UniqResult:
    keys: DeviceBuffer
    pos: DeviceBuffer
    pos_bytes: int
    n: int
    k: int


def rle_uniq(km: Kmers, dev: Device) -> UniqResult:
    if km.pos is None:
        raise ValueError("uniq needs the pos payload (extract with want_pos=True)")
    okeys = dev.alloc(8 * max(km.n, 1))
    opos = dev.alloc(km.pos_bytes * max(km.n, 1))
    if not km.sorted:
        _sort_prefix(km, dev, 2 * km.k)
        n = _finish(km, dev, 2 * km.k, N.KMAN_FINISH_UNIQ, okeys, opos, km.pos_bytes)
        return UniqResult(okeys, opos, km.pos_bytes, n, km.k)
    out = c_uint64(0)
    N.check(dev.ctx, N.lib().kman_rle_uniq(dev.ctx, c_void_p(km.keys.ptr), c_void_p(km.pos.ptr), km.pos_bytes,
                                            km.n, c_void_p(okeys.ptr), c_void_p(opos.ptr), byref(out)),
            "kman_rle_uniq")
    return UniqResult(okeys, opos, km.pos_bytes, int(out.value), km.k)


def groups(p: Parsed, k: int, rc: bool, mode: str, canonical: bool = False, mixed: bool = False):
    """kman_groups: count / uniq of the whole stream straight from the codes
    (region.h).  Returns a CountResult / UniqResult, or None when the input
    is outside the region path (kman_groups_plan / a region overflow said
    KMAN_EFALLBACK): the caller then runs extract_sorted + rle_*."""
    L, dev = N.lib(), p.dev
    m = N.KMAN_FINISH_UNIQ if mode == "uniq" else N.KMAN_FINISH_COUNT
    flags = flags_for(rc, mode == "uniq", canonical, mixed)
    wb = c_uint64(0)
    rc_ = L.kman_groups_plan(p.n_bases, k, flags, m, byref(wb))
    if rc_ == N.KMAN_EFALLBACK:
        return None
    N.check(dev.ctx, rc_, "kman_groups_plan")
    cap = max(1, p.n_bases * (2 if rc and not canonical else 1))
    vb = (4 if 2 * p.n_bases <= 0xFFFFFFFF else 8) if mode == "uniq" else (4 if cap <= 0xFFFFFFFF else 8)
    with dev.scratch() as s:
        work = s.alloc(int(wb.value))
        okeys = s.alloc(8 * cap)
        ovals = s.alloc(vb * cap)
        phases.mark("groups_alloc")
        nk, no = c_uint64(0), c_uint64(0)
        rc_ = L.kman_groups(dev.ctx, c_void_p(p.codes.ptr), p.n_bases, k, flags, m, c_void_p(work.ptr), wb.value,
                            c_void_p(okeys.ptr), c_void_p(ovals.ptr), vb, byref(nk), byref(no))
        s.keep(work).free()
        phases.mark("groups_kernels")
        if rc_ == N.KMAN_EFALLBACK:
            return None
        N.check(dev.ctx, rc_, "kman_groups")
        s.keep(okeys), s.keep(ovals)
    if mode == "uniq":
        return UniqResult(okeys, ovals, vb, int(no.value), k)
    return CountResult(okeys, ovals, vb, int(no.value), k)
