"""Reads against a count table: screen, window counts, quantile, solid runs, correction."""

from __future__ import annotations

from ctypes import byref, c_uint64, c_void_p
from typing import Optional

import numpy as np

from .. import _native as N
from .device import DeviceBuffer
from .parsed import Parsed, _rec_seq
from .kmers import CountResult
from .output import _format, _to
from .tables import _check_key_k, _index, _index_bits


def screen(p: Parsed, table: CountResult, canonical: bool = False, index: Optional[DeviceBuffer] = None,
           index_bits: Optional[int] = None) -> np.ndarray:
    """kman_screen_records: for every record of p, (valid k-mer windows, those
    whose key is a row of `table`, the sum of those rows' counts), k =
    table.k, as an (n_records, 3) u64 array.  canonical: the windows' keys are
    min(k-mer, reverse complement), for a table counted that way.  `index`: a
    table_index(dev, table, index_bits) kept by the caller (index_bits is then
    the width it was built with; None: the default width); None: built and
    freed here."""
    _check_key_k(table.k, "screen")
    dev, k, R = p.dev, table.k, int(p.n_records)
    bits = _index_bits(table, index_bits)
    if R == 0:
        return np.zeros((0, 3), np.uint64)
    with dev.scratch() as s:
        index = _index(s, table, index, bits)
        d_rec, _ = _rec_seq(s, p)
        d_out = s.alloc(24 * R)
        N.check(dev.ctx, N.lib().kman_screen_records(
            dev.ctx, c_void_p(p.codes.ptr), p.n_bases, k, N.KMAN_CANONICAL if canonical else 0, c_void_p(d_rec.ptr), R,
            c_void_p(table.ukeys.ptr), c_void_p(table.counts.ptr), table.count_bytes, table.n, c_void_p(index.ptr),
            bits, c_void_p(d_out.ptr)), "kman_screen_records")
        planes = dev.download(d_out, 3 * R, np.uint64)
    return np.ascontiguousarray(planes.reshape(3, R).T)


def window_counts(p: Parsed, table: CountResult, canonical: bool = False, index: Optional[DeviceBuffer] = None,
                  index_bits: Optional[int] = None) -> DeviceBuffer:
    """kman_window_counts: one u32 per base of p in a fresh device buffer (the
    caller frees it): the count in `table` of the k-mer window that starts at
    that base (0: not a row; counts above 0xFFFFFFFE saturate there),
    N.KMAN_WC_NONE where no valid window starts.  canonical, index, index_bits
    as for screen()."""
    _check_key_k(table.k, "window_counts")
    dev, k = p.dev, table.k
    bits = _index_bits(table, index_bits)
    with dev.scratch() as s:
        index = _index(s, table, index, bits)
        d_wc = s.alloc(max(16, 4 * int(p.n_bases)))
        N.check(dev.ctx, N.lib().kman_window_counts(
            dev.ctx, c_void_p(p.codes.ptr), p.n_bases, k, N.KMAN_CANONICAL if canonical else 0,
            c_void_p(table.ukeys.ptr), c_void_p(table.counts.ptr), table.count_bytes, table.n, c_void_p(index.ptr),
            bits, c_void_p(d_wc.ptr)), "kman_window_counts")
        return s.keep(d_wc)


def quantile_plan(rec_seq, n_bases: int):
    """(records longer than KMAN_QUANTILE_REC_CAP bases, the bases they hold
    together) of a record table, as kman_record_quantile clamps and cuts it:
    the arguments of kman_record_quantile_plan."""
    rs = np.minimum(np.asarray(rec_seq, dtype=np.uint64), np.uint64(n_bases))
    if rs.size == 0:
        return 0, 0
    ends = np.concatenate([rs[1:], np.asarray([n_bases], dtype=np.uint64)])
    lens = np.where(ends > rs, ends - rs, np.uint64(0))
    long_ = lens > np.uint64(N.KMAN_QUANTILE_REC_CAP)
    return int(long_.sum()), int(lens[long_].sum())


def record_quantile(p: Parsed, d_wc: DeviceBuffer, num: int = 1, den: int = 2) -> np.ndarray:
    """kman_record_quantile over window_counts()'s words: per record of p, the
    word of rank floor((w - 1) * num / den) among its w words that are not
    KMAN_WC_NONE, ascending (1/2: the lower median, 0/1: the minimum, 1/1: the
    maximum), 0 for a record without windows; u32, n_records.  d_wc is
    scratch afterwards (still the caller's to free)."""
    for v in (num, den):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
            raise AssertionError("quantile %r / %r: integers" % (num, den))
    if not (1 <= den <= 65535 and 0 <= num <= den):
        raise AssertionError("quantile %r / %r: 1 <= den <= 65535 and 0 <= num <= den" % (num, den))
    dev, R = p.dev, int(p.n_records)
    if R == 0:
        return np.zeros(0, np.uint32)
    with dev.scratch() as s:
        d_rec, rec_seq = _rec_seq(s, p)
        n_long, n_values = quantile_plan(rec_seq, int(p.n_bases))
        need = c_uint64(0)
        N.check(dev.ctx, N.lib().kman_record_quantile_plan(n_long, n_values, byref(need)), "kman_record_quantile_plan")
        d_work = s.alloc(need.value)
        d_q = s.alloc(max(16, 4 * R))
        N.check(dev.ctx, N.lib().kman_record_quantile(
            dev.ctx, c_void_p(d_wc.ptr), p.n_bases, c_void_p(d_rec.ptr), R, int(num), int(den), c_void_p(d_work.ptr),
            need.value, c_void_p(d_q.ptr)), "kman_record_quantile")
        return dev.download(d_q, R, np.uint32)


def screen_median(p: Parsed, table: CountResult, canonical: bool = False, index: Optional[DeviceBuffer] = None,
                  index_bits: Optional[int] = None, num: int = 1, den: int = 2):
    """(stats, median): screen()'s rows, from kman_screen_records exactly as
    screen() gets them, and record_quantile(num, den) of the records' window
    counts (u32, n_records).  The table's index is built once (or taken from
    the caller) and used by both kernels."""
    _check_key_k(table.k, "screen")
    bits = _index_bits(table, index_bits)
    with p.dev.scratch() as s:
        index = _index(s, table, index, bits)
        stats = screen(p, table, canonical, index=index, index_bits=bits)
        d_wc = s.own(window_counts(p, table, canonical, index=index, index_bits=bits))
        return stats, record_quantile(p, d_wc, num, den)


def _check_min_count(min_count) -> int:
    if isinstance(min_count, bool) or not isinstance(min_count, (int, np.integer)) or \
            not 1 <= min_count <= N.KMAN_WC_NONE - 1:
        raise AssertionError("min_count must be an integer in [1, %d], got %r" % (N.KMAN_WC_NONE - 1, min_count))
    return int(min_count)


def record_runs(p: Parsed, d_wc: DeviceBuffer, min_count: int) -> np.ndarray:
    """kman_record_runs over window_counts()'s words: per record of p, (start,
    len) of its longest run of solid bases (word != KMAN_WC_NONE and >=
    min_count): len in windows, start the offset from the record's first base
    of the leftmost run of that length, both 0 for a record without a solid
    base; an (n_records, 2) u64 array.  d_wc is not modified."""
    min_count = _check_min_count(min_count)
    dev, R = p.dev, int(p.n_records)
    if R == 0:
        return np.zeros((0, 2), np.uint64)
    need = c_uint64(0)
    N.check(dev.ctx, N.lib().kman_record_runs_plan(int(p.n_bases), R, byref(need)), "kman_record_runs_plan")
    with dev.scratch() as s:
        d_rec, _ = _rec_seq(s, p)
        d_work = s.alloc(need.value)
        d_out = s.alloc(16 * R)
        N.check(dev.ctx, N.lib().kman_record_runs(
            dev.ctx, c_void_p(d_wc.ptr), p.n_bases, c_void_p(d_rec.ptr), R, min_count, c_void_p(d_work.ptr),
            need.value, c_void_p(d_out.ptr)), "kman_record_runs")
        planes = dev.download(d_out, 2 * R, np.uint64)
    return np.ascontiguousarray(planes.reshape(2, R).T)


def solid_spans(runs, k: int):
    """(START, END) of record_runs()'s rows in bases within the record, as
    `codes` holds them (every sequence character counts, N included; line
    breaks do not): START = start, END = start + len + k - 1 where len > 0 (a
    run of len windows covers len + k - 1 bases), both 0 otherwise."""
    runs = np.asarray(runs, dtype=np.uint64).reshape(-1, 2)
    has = runs[:, 1] > 0
    start = np.where(has, runs[:, 0], np.uint64(0)).astype(np.uint64)
    end = np.where(has, runs[:, 0] + runs[:, 1] + np.uint64(int(k) - 1), np.uint64(0)).astype(np.uint64)
    return np.ascontiguousarray(start), np.ascontiguousarray(end)


def screen_solid(p: Parsed, table: CountResult, canonical: bool, min_count: int, *, median: bool = False,
                 index: Optional[DeviceBuffer] = None, index_bits: Optional[int] = None):
    """(stats, median or None, runs): screen()'s rows, record_quantile()'s
    lower median when `median`, and record_runs(min_count) of the records'
    window counts.  The table's index is built once (or taken from the caller)
    and serves every kernel; window_counts runs once, and the runs are taken
    before the quantile, which leaves the words as scratch."""
    _check_key_k(table.k, "screen")
    min_count = _check_min_count(min_count)
    bits = _index_bits(table, index_bits)
    with p.dev.scratch() as s:
        index = _index(s, table, index, bits)
        stats = screen(p, table, canonical, index=index, index_bits=bits)
        d_wc = s.own(window_counts(p, table, canonical, index=index, index_bits=bits))
        runs = record_runs(p, d_wc, min_count)
        med = record_quantile(p, d_wc) if median else None
        return stats, med, runs


def correct(p: Parsed, table: CountResult, canonical: bool, min_count: int, *, index: Optional[DeviceBuffer] = None,
            index_bits: Optional[int] = None, d_wc: Optional[DeviceBuffer] = None) -> np.ndarray:
    """Isolated substitution errors of p's records put right against `table`
    (kman_correct_sites, kman_apply_fixes; the rule: include/kman.h): a run of
    at most k window counts below min_count with a count >= min_count next to
    it names one base, and the base is replaced when exactly one other base
    makes every window over it reach min_count.  ``p.codes`` is patched in
    place, and ``p.text`` (four-line FASTQ) when the parse kept it; quality
    values never change.  Returns the fixes per record, u32.  `d_wc`:
    window_counts() of p as it is, kept by the caller (not modified; stale
    afterwards where a base changed); None: computed and freed here.  One
    pass: the corrected records are not examined again.  index, index_bits as
    for screen()."""
    _check_key_k(table.k, "correct")
    min_count = _check_min_count(min_count)
    dev, k, R, n = p.dev, table.k, int(p.n_records), int(p.n_bases)
    bits = _index_bits(table, index_bits)
    if R == 0 or n == 0:
        return np.zeros(R, np.uint32)
    with dev.scratch() as s:
        index = _index(s, table, index, bits)
        if d_wc is None:
            d_wc = s.own(window_counts(p, table, canonical, index=index, index_bits=bits))
        d_rec, _ = _rec_seq(s, p)
        d_fix = s.alloc(max(16, n))
        n_fixed = c_uint64(0)
        N.check(dev.ctx, N.lib().kman_correct_sites(
            dev.ctx, c_void_p(p.codes.ptr), n, k, N.KMAN_CANONICAL if canonical else 0, c_void_p(d_wc.ptr),
            c_void_p(d_rec.ptr), R, c_void_p(table.ukeys.ptr), c_void_p(table.counts.ptr), table.count_bytes, table.n,
            c_void_p(index.ptr), bits, min_count, c_void_p(d_fix.ptr), byref(n_fixed)), "kman_correct_sites")
        d_text = d_off = None
        if p.text is not None:
            off = np.empty(R + 1, dtype=np.uint64)
            off[:R] = p.rec_hdr
            off[R] = int(p.text_bytes)
            d_off = s.alloc(off.nbytes)
            dev.upload(d_off, off)
            d_text = p.text
        d_nfix = s.alloc(max(16, 4 * R))
        N.check(dev.ctx, N.lib().kman_apply_fixes(
            dev.ctx, c_void_p(p.codes.ptr), n, c_void_p(d_fix.ptr), c_void_p(d_rec.ptr), R,
            c_void_p(d_text.ptr) if d_text is not None else None, int(p.text_bytes) if d_text is not None else 0,
            c_void_p(d_off.ptr) if d_off is not None else None, c_void_p(d_nfix.ptr)), "kman_apply_fixes")
        return dev.download(d_nfix, R, np.uint32)


def _keep_array(keep, R: int):
    if keep is None:
        return None
    keep = np.ascontiguousarray(keep, dtype=np.uint8)
    if keep.shape != (R,):
        raise AssertionError("keep mask of %r for %d records" % (keep.shape, R))
    return keep


def _span_arrays(span, R: int):
    start, end = (np.ascontiguousarray(np.asarray(a, dtype=np.uint64).reshape(-1)) for a in span)
    if start.shape != (R,) or end.shape != (R,):
        raise AssertionError("span arrays of %r and %r for %d records" % (start.shape, end.shape, R))
    return start, end


def screen_keep(stats: np.ndarray, min_hits: int = 0, min_frac: float = 0.0, invert: bool = False, *, median=None,
                min_median: Optional[int] = None, max_median: Optional[int] = None, span=None,
                min_solid_len: Optional[int] = None) -> np.ndarray:
    """Which records of screen()'s rows are written, a u8 mask: those with
    hits >= min_hits and hits >= min_frac * windows (float64) and, with
    `median` (screen_median()'s second result), min_median <= median <=
    max_median (each bound only when given) and, with `span` (solid_spans()'s
    pair), END - START >= min_solid_len (when given), the others when
    `invert`."""
    stats = np.asarray(stats, dtype=np.uint64).reshape(-1, 3)
    windows, hits = stats[:, 0].astype(np.float64), stats[:, 1].astype(np.float64)
    keep = (hits >= min_hits) & (hits >= min_frac * windows)
    if min_median is not None or max_median is not None:
        if median is None:
            raise AssertionError("min_median / max_median need the median array")
        med = np.asarray(median, dtype=np.uint32).reshape(-1).astype(np.int64)
        if med.shape[0] != stats.shape[0]:
            raise AssertionError("%d medians for %d records" % (med.shape[0], stats.shape[0]))
        if min_median is not None:
            keep &= med >= min(int(min_median), 1 << 40)  # (bounds outside u32 clipped into int64)
        if max_median is not None:
            keep &= med <= max(int(max_median), -1)
    if min_solid_len is not None:
        if span is None:
            raise AssertionError("min_solid_len needs the span arrays")
        start, end = _span_arrays(span, stats.shape[0])
        keep &= (end - np.minimum(start, end)).astype(np.float64) >= float(min_solid_len)
    if invert:
        keep = ~keep
    return keep.astype(np.uint8)


def emit_screen(p: Parsed, stats: np.ndarray, keep, sink=None, median=None, *, span=None, fixes=None):
    """The `kmer screen` text of screen()'s rows: one "name<TAB>windows<TAB>
    hits<TAB>sum" line per record with keep != 0 (None: all), in input order
    (kman_format_screen); with `median` (u32 per record) a fifth column
    "<TAB>median" (kman_format_screen_median); with `span` (solid_spans()'s
    pair) two last columns "<TAB>START<TAB>END" (kman_format_screen_solid);
    with `fixes` (correct()'s array; needs `span`) one more, "<TAB>FIXES"
    (kman_format_screen_correct).  Returned, or written to the binary file
    `sink`."""
    stats = np.asarray(stats, dtype=np.uint64).reshape(-1, 3)
    R = stats.shape[0]
    if R != p.n_records:
        raise AssertionError("%d rows for %d records" % (R, p.n_records))
    planes = np.ascontiguousarray(stats.T)
    off = np.ascontiguousarray(p.name_off, dtype=np.uint64)
    keep = _keep_array(keep, R)
    kp = keep.ctypes.data_as(c_void_p) if keep is not None else None
    if median is not None:
        median = np.ascontiguousarray(median, dtype=np.uint32)
        if median.shape != (R,):
            raise AssertionError("median array of %r for %d records" % (median.shape, R))
    if fixes is not None:
        if span is None:
            raise AssertionError("fixes need the span arrays")
        fixes = np.ascontiguousarray(fixes, dtype=np.uint32)
        if fixes.shape != (R,):
            raise AssertionError("fixes array of %r for %d records" % (fixes.shape, R))
        start, end = _span_arrays(span, R)
        mp = median.ctypes.data_as(c_void_p) if median is not None else None
        return _to(sink, _format(N.lib().kman_format_screen_correct, planes.ctypes.data_as(c_void_p), mp,
                                 start.ctypes.data_as(c_void_p), end.ctypes.data_as(c_void_p),
                                 fixes.ctypes.data_as(c_void_p), R, kp, p.names_blob, off.ctypes.data_as(c_void_p)))
    if span is not None:
        start, end = _span_arrays(span, R)
        mp = median.ctypes.data_as(c_void_p) if median is not None else None
        return _to(sink, _format(N.lib().kman_format_screen_solid, planes.ctypes.data_as(c_void_p), mp,
                                 start.ctypes.data_as(c_void_p), end.ctypes.data_as(c_void_p), R, kp, p.names_blob,
                                 off.ctypes.data_as(c_void_p)))
    if median is not None:
        return _to(sink, _format(N.lib().kman_format_screen_median, planes.ctypes.data_as(c_void_p),
                                 median.ctypes.data_as(c_void_p), R, kp, p.names_blob, off.ctypes.data_as(c_void_p)))
    return _to(sink, _format(N.lib().kman_format_screen, planes.ctypes.data_as(c_void_p), R, kp, p.names_blob,
                             off.ctypes.data_as(c_void_p)))


def emit_bed(p: Parsed, span, keep, sink=None):
    """The BED of the solid spans: one "name<TAB>START<TAB>END" line per
    record with keep != 0 (None: all) and END > START, in input order
    (kman_format_bed).  Returned, or written to the binary file `sink`."""
    R = int(p.n_records)
    start, end = _span_arrays(span, R)
    off = np.ascontiguousarray(p.name_off, dtype=np.uint64)
    keep = _keep_array(keep, R)
    kp = keep.ctypes.data_as(c_void_p) if keep is not None else None
    return _to(sink, _format(N.lib().kman_format_bed, start.ctypes.data_as(c_void_p), end.ctypes.data_as(c_void_p), R,
                             kp, p.names_blob, off.ctypes.data_as(c_void_p)))
