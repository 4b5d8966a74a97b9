"""The resident pipeline: one text in HBM, every buffer preallocated."""

from __future__ import annotations

import ctypes
from ctypes import byref, c_int, c_uint64, c_void_p
from typing import Optional

from .. import _native as N
from .device import Device, free_all
from .kmers import _check_k, flags_for, split_bits


class ResidentPipeline:
    """One FASTA text resident in HBM, every buffer preallocated: ``step()``
    runs parse -> extract -> sort -> count|uniq with no allocation, leaving
    the result device-resident (what bench.py times)."""

    def __init__(self, dev: Device, text: bytes, k: int, mode: str = "uniq", rc: bool = False,
                 pos_bytes: Optional[int] = None, path: str = "region"):
        _check_k(k)
        if mode not in ("count", "uniq"):
            raise ValueError(mode)
        if path not in ("region", "split", "full"):
            raise ValueError(path)
        # region: kman_groups (default; falls back to split when the input is
        # outside the region path); split: prefix passes + kman_finish; full:
        # every bit in global passes + kman_rle_* (kept for A/B runs)
        self.path = path
        self.work = None
        self.dev, self.k, self.mode, self.rc = dev, k, mode, rc
        n = len(text)
        self.n_bytes = n
        self.text = dev.alloc(n + 64)
        dev.upload(self.text, text)
        self.codes = dev.alloc(n + 64)
        self.rec_cap = n // 2 + 1
        self.rec_hdr = dev.alloc(8 * self.rec_cap)
        self.rec_seq = dev.alloc(8 * self.rec_cap)
        self.bound = max(1, n * (2 if rc else 1))
        self.pos_bytes = pos_bytes or (4 if 2 * n <= 0xFFFFFFFF else 8)
        want_pos = mode == "uniq"
        self.keys = dev.alloc(8 * self.bound)
        self.alt = dev.alloc(8 * self.bound)
        self.pos = dev.alloc(self.pos_bytes * self.bound) if want_pos else None
        self.pos_alt = dev.alloc(self.pos_bytes * self.bound) if want_pos else None
        self.hist = dev.alloc(8 * 256 * 8)
        self.out_keys = dev.alloc(8 * self.bound)
        self.count_bytes = 4 if self.bound <= 0xFFFFFFFF else 8
        self.out_vals = dev.alloc((self.pos_bytes if want_pos else self.count_bytes) * self.bound)
        self.lo_bit = split_bits(self.bound, 2 * k) if path == "split" else 0
        self.flags = flags_for(rc, want_pos) | N.KMAN_HIST_LO(self.lo_bit)
        self.n_kmers = 0
        self.n_out = 0
        self.n_bases = 0
        self.sorted_in_alt = False
        if self.path == "region":
            self._parse()
            wb = c_uint64(0)
            m = N.KMAN_FINISH_UNIQ if mode == "uniq" else N.KMAN_FINISH_COUNT
            r = N.lib().kman_groups_plan(self.n_bases, k, flags_for(rc, want_pos), m, byref(wb))
            if r == N.KMAN_EFALLBACK:
                self._to_split()
            else:
                N.check(dev.ctx, r, "kman_groups_plan")
                self.work = dev.alloc(int(wb.value))
                self.work_bytes = int(wb.value)

    def _to_split(self) -> None:
        """Switch to the prefix-split path with its own digit plan (the region
        path plans no prefix passes: lo_bit 0 would run every key bit through
        the global passes)."""
        self.path = "split"
        if self.work is not None:
            self.work.free()
            self.work = None
        self.lo_bit = split_bits(self.bound, 2 * self.k)
        self.flags = flags_for(self.rc, self.mode == "uniq") | N.KMAN_HIST_LO(self.lo_bit)

    def _parse(self) -> None:
        info = N.ParseInfo()
        N.check(self.dev.ctx, N.lib().kman_parse_fasta(self.dev.ctx, c_void_p(self.text.ptr), self.n_bytes,
                                                        c_void_p(self.codes.ptr), c_void_p(self.rec_hdr.ptr),
                                                        c_void_p(self.rec_seq.ptr), self.rec_cap, byref(info)),
                "kman_parse_fasta")
        self.n_bases = int(info.n_bases)

    def extract_only(self) -> int:
        """parse + extract (stream-order keys / pos in self.keys / self.pos)."""
        L, ctx = N.lib(), self.dev.ctx
        self._parse()
        n = c_uint64(0)
        pos = c_void_p(self.pos.ptr) if self.pos else c_void_p(None)
        N.check(ctx, L.kman_extract(ctx, c_void_p(self.codes.ptr), self.n_bases, self.k, self.flags,
                                    c_void_p(self.keys.ptr), pos, self.pos_bytes, self.bound, None, byref(n)),
                "kman_extract")
        self.n_kmers = int(n.value)
        return self.n_kmers

    def step(self) -> int:
        L, ctx = N.lib(), self.dev.ctx
        self._parse()
        if self.path == "region":
            m = N.KMAN_FINISH_UNIQ if self.mode == "uniq" else N.KMAN_FINISH_COUNT
            ob = self.count_bytes if self.mode == "count" else self.pos_bytes
            nk, no = c_uint64(0), c_uint64(0)
            r = L.kman_groups(ctx, c_void_p(self.codes.ptr), self.n_bases, self.k, self.flags & 0xff, m,
                              c_void_p(self.work.ptr), self.work_bytes, c_void_p(self.out_keys.ptr),
                              c_void_p(self.out_vals.ptr), ob, byref(nk), byref(no))
            if r != N.KMAN_EFALLBACK:
                N.check(ctx, r, "kman_groups")
                self.n_kmers, self.n_out = int(nk.value), int(no.value)
                return self.n_kmers
            # a region overflowed (skewed input): the general path from here on
            self._to_split()
        n = c_uint64(0)
        res = c_int(0)
        pos = c_void_p(self.pos.ptr) if self.pos else c_void_p(None)
        vb = self.pos_bytes if self.pos else 0
        pos_alt = c_void_p(self.pos_alt.ptr if self.pos_alt else None)
        if self.path == "split":
            # extraction fused with the first prefix pass, then the other prefix passes
            N.check(ctx, L.kman_extract_sorted(ctx, c_void_p(self.codes.ptr), self.n_bases, self.k,
                                               self.flags & 0xff, self.lo_bit, c_void_p(self.keys.ptr),
                                               c_void_p(self.alt.ptr), pos, pos_alt, self.pos_bytes, self.bound,
                                               byref(n), byref(res)), "kman_extract_sorted")
            self.n_kmers = int(n.value)
        else:
            N.check(ctx, L.kman_memset(ctx, c_void_p(self.hist.ptr), 0, 8 * 256 * 8), "memset")
            N.check(ctx, L.kman_extract(ctx, c_void_p(self.codes.ptr), self.n_bases, self.k, self.flags,
                                        c_void_p(self.keys.ptr), pos, self.pos_bytes, self.bound,
                                        c_void_p(self.hist.ptr), byref(n)), "kman_extract")
            self.n_kmers = int(n.value)
            N.check(ctx, L.kman_sort(ctx, c_void_p(self.keys.ptr), c_void_p(self.alt.ptr), pos, pos_alt, vb,
                                     self.n_kmers, 2 * self.k, c_void_p(self.hist.ptr), byref(res)), "kman_sort")
        self.sorted_in_alt = bool(res.value)
        skeys = self.alt if res.value else self.keys
        out = c_uint64(0)
        if self.path == "split":
            spos = self.pos_alt if res.value else self.pos
            other = self.keys if res.value else self.alt
            opos = self.pos if res.value else self.pos_alt
            mode = N.KMAN_FINISH_COUNT if self.mode == "count" else N.KMAN_FINISH_UNIQ
            ob = self.count_bytes if self.mode == "count" else self.pos_bytes
            N.check(ctx, L.kman_finish(ctx, c_void_p(skeys.ptr), c_void_p(other.ptr),
                                       c_void_p(spos.ptr if spos else None), c_void_p(opos.ptr if opos else None), vb,
                                       self.n_kmers, 2 * self.k, self.lo_bit, mode, c_void_p(self.out_keys.ptr),
                                       c_void_p(self.out_vals.ptr), ob, byref(out)), "kman_finish")
        elif self.mode == "count":
            N.check(ctx, L.kman_rle_count(ctx, c_void_p(skeys.ptr), self.n_kmers, c_void_p(self.out_keys.ptr),
                                          c_void_p(self.out_vals.ptr), self.count_bytes, byref(out)),
                    "kman_rle_count")
        else:
            spos = self.pos_alt if res.value else self.pos
            N.check(ctx, L.kman_rle_uniq(ctx, c_void_p(skeys.ptr), c_void_p(spos.ptr), self.pos_bytes,
                                         self.n_kmers, c_void_p(self.out_keys.ptr), c_void_p(self.out_vals.ptr),
                                         byref(out)), "kman_rle_uniq")
        self.n_out = int(out.value)
        return self.n_kmers

    @property
    def n_sorted(self) -> int:
        return self.n_kmers

    def timing(self, enable: bool) -> None:
        N.check(self.dev.ctx, N.lib().kman_timing_enable(self.dev.ctx, 1 if enable else 0), "timing")

    def timed(self, tag: str):
        n, ms = c_uint64(0), ctypes.c_double(0)
        N.check(self.dev.ctx, N.lib().kman_timing_query(self.dev.ctx, tag.encode(), byref(n), byref(ms)), "timing")
        return int(n.value), float(ms.value)

    def free(self) -> None:
        free_all(self.text, self.codes, self.rec_hdr, self.rec_seq, self.keys, self.alt, self.pos, self.pos_alt,
                 self.hist, self.out_keys, self.out_vals, self.work)
