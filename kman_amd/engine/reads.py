"""Whole reads: the record cutter, homopolymer compression and read pairs."""

from __future__ import annotations

from ctypes import byref, c_uint64, c_void_p
from typing import Optional

import numpy as np

from .. import _native as N
from .. import phases
from . import device
from .device import BorrowedBuffer, DeviceBuffer
from .parsed import BlobNames, Parsed
from .kmers import CountResult
from .output import _format, _format_dev, _to, host_format
from .tables import _check_key_k, _index, _index_bits
from .lookup import (
    _check_min_count, _keep_array, _span_arrays, emit_screen, record_quantile, record_runs, screen, window_counts,
)


_CUT_MAX_RECORDS = 1 << 24  # records per slice of cut_records (its work memory: 16 B each, 64 B under trim)


def _cut_slices(bound: np.ndarray, limit: int):
    """(i0, records, text bound) per slice: as many records as fit `limit`
    bytes of text bound (at most _CUT_MAX_RECORDS), at least one, so a record
    larger than `limit` gets a slice of its own."""
    cum = np.cumsum(bound, dtype=np.uint64)
    R, i0, done, res = len(bound), 0, 0, []
    while i0 < R:
        j = int(np.searchsorted(cum, np.uint64(done + limit), side="right"))
        j = min(max(j, i0 + 1), i0 + _CUT_MAX_RECORDS, R)
        res.append((i0, j - i0, int(cum[j - 1]) - done))
        i0, done = j, int(cum[j - 1])
    return res


def cut_records(p: Parsed, keep, sink=None, *, span=None, trim=False):
    """The text of the records of p with keep != 0 (None: all), in input order
    (kman_cut_records), from the device text that parse(..., keep_text=True)
    left in ``p.text``: record r is the input's bytes from rec_hdr[r] to
    rec_hdr[r + 1] (the last one runs to the text's end), verbatim.  With
    `trim` (FASTQ records; `span`: solid_spans()'s pair) every record is cut to
    its columns [START, END): header, sequence[START:END], the ``+`` line and
    quality[START:END], each followed by ``"\\n"``; a record with END <= START
    is left out.  Returned (a bytearray), or written to the binary file `sink`,
    through _format_dev's pinned stages and writer pool, in slices of whole
    records chosen from rec_hdr (a record's text is at most its bytes + 4); a
    record larger than a slice gets a slice, and stages, sized for it."""
    if p.text is None:
        raise AssertionError("cut_records needs the input text on the device: parse with keep_text=True")
    dev, L, R, n = p.dev, N.lib(), int(p.n_records), int(p.text_bytes)
    keep = _keep_array(keep, R)
    if trim and span is None:
        raise AssertionError("trim needs the span arrays")
    if span is not None and not trim:
        raise AssertionError("span arrays are for trim=True")
    if R == 0:
        return None if sink is not None else bytearray()
    off = np.empty(R + 1, dtype=np.uint64)
    off[:R] = p.rec_hdr
    off[R] = n
    ends = np.minimum(off[1:], np.uint64(n)).astype(np.int64)
    bound = np.maximum(ends - np.minimum(off[:R], np.uint64(n)).astype(np.int64), 0) + 4
    if keep is not None:
        bound[keep == 0] = 0
    slices = _cut_slices(bound, device._FMT_SLICE)
    flags = N.KMAN_CUT_TRIM if trim else 0
    need = c_uint64(0)
    N.check(dev.ctx, L.kman_cut_records_plan(max(m for _, m, _ in slices), flags, byref(need)),
            "kman_cut_records_plan")
    with dev.scratch() as s:
        def up(a):
            b = s.alloc(a.nbytes)
            dev.upload(b, a)
            return b.ptr

        d_off = up(off)
        d_keep = up(keep) if keep is not None else None
        d_start = d_end = None
        if trim:
            start, end = _span_arrays(span, R)
            d_start, d_end = up(start), up(end)
        d_work = s.alloc(need.value)

        def at(ptr, nbytes):
            return c_void_p(ptr + nbytes) if ptr is not None else None

        def call(i0, m, d_out, cap, used):
            return L.kman_cut_records(dev.ctx, c_void_p(p.text.ptr), n, at(d_off, 8 * i0), m, at(d_keep, i0),
                                      at(d_start, 8 * i0), at(d_end, 8 * i0), flags, c_void_p(d_work.ptr), need.value,
                                      d_out, cap, byref(used))

        return _format_dev(dev, R, 0, call, sink, slices=slices)


def _cut_host(text: bytes, off, keep, span, trim: bool) -> bytes:
    """cut_records' bytes by a plain host loop (KMAN_HOST_FORMAT)."""
    import re

    out = []
    for r in range(len(off) - 1):
        if keep is not None and not keep[r]:
            continue
        rec = text[int(off[r]):int(off[r + 1])]
        if not trim:
            out.append(rec)
            continue
        s, e = int(span[0][r]), int(span[1][r])
        lines = (re.split(rb"\r\n|\n|\r", rec) + [b""] * 4)[:4]
        body = lines[1].rstrip(b" \t\n\r\v\f\x1c\x1d\x1e\x1f")
        cols = [c for c in range(len(body)) if body[c] not in b" \r"]
        e = min(e, len(cols))
        if s >= e:
            continue
        c0, c1 = cols[s], cols[e - 1] + 1
        out.append(lines[0] + b"\n" + lines[1][c0:c1] + b"\n" + lines[2] + b"\n" + lines[3][c0:c1] + b"\n")
    return b"".join(out)


def emit_reads(p: Parsed, keep, sink, *, span=None, trim=False):
    """`kmer screen --reads-out`: cut_records of the listed records; under
    `trim` the listed records without a stretch (END == START) are left out,
    as emit_bed leaves them out.  KMAN_HOST_FORMAT=1: a host loop over the
    downloaded text instead of the device kernels."""
    R = int(p.n_records)
    keep = _keep_array(keep, R)
    if trim:
        if span is None:
            raise AssertionError("trim needs the span arrays")
        start, end = _span_arrays(span, R)
        keep = (np.ones(R, np.uint8) if keep is None else keep.copy())
        keep[end == start] = 0
        span = (start, end)
    if host_format():
        if p.text is None:
            raise AssertionError("emit_reads needs the input text on the device: parse with keep_text=True")
        text = p.dev.download(p.text, p.text_bytes, np.uint8).tobytes()
        off = list(p.rec_hdr) + [p.text_bytes]
        return _to(sink, _cut_host(text, off, keep, span, trim))
    return cut_records(p, keep, sink, span=span, trim=trim)


# ------------------------------------------------- homopolymer compression
#
# One more transformation of the parsed codes, like the -q mask and the mate
# zip: every run of one base collapses to its first base (kman_hpc_records;
# the rule: include/kman.h).  Everything downstream takes the new Parsed.


def hpc(p: Parsed, *, keep_map: bool = False) -> Parsed:
    """p with homopolymer-compressed codes (kman_hpc_records): a new Parsed
    with the kept codes (a record's first base, N and other letters and bases
    masked by -q are always kept, so the mask is applied before the
    compression), the new ``rec_seq`` and ``n_bases`` and p's names,
    ``rec_hdr``, ``text`` and ``text_bytes``, so cut_records still writes the
    original records.  `keep_map`: the result also carries ``hpc_orig`` (the
    original index of every kept base, u64 on the device), ``hpc_rec_seq`` and
    ``hpc_n_bases`` (p's own), for hpc_spans.  ``p.codes`` is freed (peak:
    twice the codes, plus 8 B per base for the map); the result owns the text
    and every buffer, and p must not be used afterwards."""
    if p.mates is not None:
        raise AssertionError("hpc takes a plain parse: compress each input before zip_pairs")
    dev, R, n = p.dev, int(p.n_records), int(p.n_bases)
    with dev.scratch() as s:
        codes, orig = s.alloc(n + 64), None
        d_rec, d_out = s.alloc(max(16, 8 * R)), s.alloc(max(16, 8 * R))
        if R:
            dev.upload(d_rec, np.ascontiguousarray(p.rec_seq, dtype=np.uint64))
        if keep_map:
            orig = s.alloc(max(16, 8 * n))
        n_out = c_uint64(0)
        N.check(dev.ctx, N.lib().kman_hpc_records(
            dev.ctx, c_void_p(p.codes.ptr), n, c_void_p(d_rec.ptr), R, c_void_p(codes.ptr), c_void_p(d_out.ptr),
            c_void_p(orig.ptr) if orig is not None else None, byref(n_out)), "kman_hpc_records")
        rec_seq = dev.download(d_out, R, np.uint64) if R else np.zeros(0, np.uint64)
        res, omap = s.keep(codes), s.keep(orig)
    p.codes.free()
    text, p.text = p.text, None
    phases.mark("hpc")
    return Parsed(dev, res, int(n_out.value), R, p.rec_hdr, rec_seq, p.names, p.names_blob, p.name_off, p.n_masked,
                  text=text, text_bytes=p.text_bytes, hpc_orig=omap,
                  hpc_rec_seq=np.ascontiguousarray(p.rec_seq, dtype=np.uint64) if keep_map else None,
                  hpc_n_bases=n if keep_map else 0)


_hpc_parsed = hpc  # (for callers whose own `hpc` argument hides the function)


def hpc_spans(p: Parsed, span):
    """(START, END) per record of hpc(keep_map=True)'s result, from compressed
    columns to the columns of the original record: START_o = orig[rs_c +
    START] - rs_o, END_o = orig[rs_c + END] - rs_o, or, when END is the
    compressed record's length, the original record's length: the whole run of
    the stretch's last base lies inside it.  A record without a stretch (END
    <= START) gets 0 and 0.  The two look-ups per record are one kman_gather
    from the device map."""
    if p.hpc_orig is None:
        raise AssertionError("hpc_spans needs the map: hpc(p, keep_map=True)")
    dev, R = p.dev, int(p.n_records)
    start, end = _span_arrays(span, R)
    if R == 0:
        return start, end
    rs_c = np.ascontiguousarray(p.rec_seq, dtype=np.uint64)
    rs_o = p.hpc_rec_seq
    end_c = np.append(rs_c[1:], np.uint64(p.n_bases))
    end_o = np.append(rs_o[1:], np.uint64(p.hpc_n_bases))
    has = (end > start) & (rs_c + end <= end_c)
    inner = has & (rs_c + end < end_c)  # END is a base of the record: its first original column ends the stretch
    idx = np.zeros(2 * R, dtype=np.uint64)
    idx[:R] = np.where(has, rs_c + start, np.uint64(0))
    idx[R:] = np.where(inner, rs_c + end, np.uint64(0))
    if not has.any():
        return np.zeros(R, np.uint64), np.zeros(R, np.uint64)
    with dev.scratch() as s:
        d_idx, d_val = s.alloc(idx.nbytes), s.alloc(idx.nbytes)
        dev.upload(d_idx, idx)
        N.check(dev.ctx, N.lib().kman_gather(dev.ctx, c_void_p(p.hpc_orig.ptr), c_void_p(d_idx.ptr), 2 * R,
                                             c_void_p(d_val.ptr), 8), "gather")
        val = dev.download(d_val, 2 * R, np.uint64)
    zero = np.uint64(0)
    s_o = np.where(has, val[:R] - rs_o, zero).astype(np.uint64)
    e_o = np.where(has, np.where(inner, val[R:], end_o) - rs_o, zero).astype(np.uint64)
    return np.ascontiguousarray(s_o), np.ascontiguousarray(e_o)


#
# Two views of one code buffer in which the mates of every pair are neighbours
# (kman_zip_records, or an interleaved input as it is parsed): the MATE VIEW
# has one record per mate, the PAIR VIEW one per pair, its table being every
# second entry of the mate view's.  The lookup kernels cut windows at bit 3 of
# the codes, so no window spans two mates in either view.


def _pair_keys(p: Parsed):
    """(bytes, starts, lengths) of p's names by the pair name rule: a name is
    ``Parsed.names[i]`` with one trailing ``/1`` or ``/2`` removed."""
    arr = np.frombuffer(p.names_blob, dtype=np.uint8)
    off = np.asarray(p.name_off, dtype=np.int64)
    ln = off[1:] - off[:-1]
    suf = np.zeros(len(ln), dtype=bool)
    two = np.nonzero(ln >= 2)[0]
    if len(two):
        last, prev = arr[off[1:][two] - 1], arr[off[1:][two] - 2]
        suf[two] = (prev == 0x2F) & ((last == 0x31) | (last == 0x32))
    return arr, off[:-1], ln - 2 * suf


def _first_name_mismatch(k1, k2) -> int:
    """The first index at which two _pair_keys differ, -1 when none does."""
    (a1, s1, l1), (a2, s2, l2) = k1, k2
    bad = np.nonzero(l1 != l2)[0]
    first = int(bad[0]) if len(bad) else len(l1)
    ln = np.where(l1 == l2, l1, 0)
    tot = int(ln.sum())
    if tot:
        base = np.cumsum(ln) - ln
        within = np.arange(tot, dtype=np.int64) - np.repeat(base, ln)
        diff = np.nonzero(a1[np.repeat(s1, ln) + within] != a2[np.repeat(s2, ln) + within])[0]
        if len(diff):
            first = min(first, int(np.searchsorted(base + ln, diff[0], side="right")))
    return first if first < len(l1) else -1


def check_pair_names(names1: Parsed, names2: Parsed) -> None:
    """Refuses (AssertionError) the first pair whose two names differ by the
    pair name rule (_pair_keys), naming the 1-based pair and both names.  Host
    code over the parses' name blobs."""
    i = _first_name_mismatch(_pair_keys(names1), _pair_keys(names2))
    if i >= 0:
        raise AssertionError("pair %d: the mates' names differ, %r and %r (a trailing /1 or /2 is ignored): the "
                             "files are not in step" % (i + 1, bytes(names1.names[i]), bytes(names2.names[i])))


def _even_names(p: Parsed):
    """(names, blob, name_off) of the records 0, 2, 4, .. of p."""
    arr = np.frombuffer(p.names_blob, dtype=np.uint8)
    off = np.asarray(p.name_off, dtype=np.int64)
    st, ln = off[:-1][0::2], (off[1:] - off[:-1])[0::2]
    tot = int(ln.sum())
    base = np.cumsum(ln) - ln
    blob = arr[np.repeat(st, ln) + (np.arange(tot, dtype=np.int64) - np.repeat(base, ln))].tobytes() if tot else b""
    name_off = np.zeros(len(ln) + 1, dtype=np.uint64)
    if len(ln):
        name_off[1:] = np.cumsum(ln, dtype=np.uint64)
    return BlobNames(blob, name_off), blob, name_off


def zip_pairs(p1: Parsed, p2: Parsed, *, check_names: bool = True) -> Parsed:
    """The mate view of two parses whose i-th records are the two mates of pair
    i (kman_zip_records): 2R records, record 2i mate 1 and record 2i + 1 mate 2
    of pair i, their codes copied verbatim (bit 3, a ``-q`` mask) into one
    fresh buffer.  Different record counts are refused, and with `check_names`
    the first pair whose names differ (check_pair_names), both before any
    device work.
    ``p1.codes`` and ``p2.codes`` are freed once the zip is done (peak: twice
    the codes).  Names, ``rec_hdr`` and the texts are not merged: the result
    has no names, and carries the two sources as ``mates`` -- with their
    names, ``rec_hdr`` and, when they were parsed with keep_text, their device
    texts, for cut_records.  ``free()`` of the result frees them too; p1 and p2
    must not be used for lookups afterwards."""
    if p1.n_records != p2.n_records:
        raise AssertionError("READS has %d records and READS2 has %d: the files are not the two ends of the same "
                             "fragments" % (p1.n_records, p2.n_records))
    if p1.dev is not p2.dev:
        raise AssertionError("zip_pairs: the two parses are on different devices")
    if check_names:
        check_pair_names(p1, p2)
    dev, R = p1.dev, int(p1.n_records)
    n = int(p1.n_bases) + int(p2.n_bases) if R else 0
    with dev.scratch() as s:
        codes = s.alloc(int(p1.n_bases) + int(p2.n_bases) + 64)
        d1, d2, d_out = s.alloc(max(16, 8 * R)), s.alloc(max(16, 8 * R)), s.alloc(max(16, 16 * R))
        if R:
            dev.upload(d1, np.ascontiguousarray(p1.rec_seq, dtype=np.uint64))
            dev.upload(d2, np.ascontiguousarray(p2.rec_seq, dtype=np.uint64))
        N.check(dev.ctx, N.lib().kman_zip_records(
            dev.ctx, c_void_p(p1.codes.ptr), int(p1.n_bases), c_void_p(d1.ptr), c_void_p(p2.codes.ptr),
            int(p2.n_bases), c_void_p(d2.ptr), R, c_void_p(codes.ptr), c_void_p(d_out.ptr)), "kman_zip_records")
        rec_seq = dev.download(d_out, 2 * R, np.uint64)
        res = s.keep(codes)
    p1.codes.free()
    p2.codes.free()
    phases.mark("zip_pairs")
    return Parsed(dev, res, n, 2 * R, np.zeros(0, np.uint64), rec_seq, [], b"", np.zeros(1, np.uint64),
                  int(p1.n_masked) + int(p2.n_masked), mates=(p1, p2))


def pair_view(pz: Parsed) -> Parsed:
    """The pair view of zip_pairs' result: the same codes with every second
    entry of its record table, so R records, each a pair; names and
    ``rec_hdr`` are mate 1's as READS has them.  The view borrows the codes
    (BorrowedBuffer): freeing it frees nothing, and it is valid only while
    `pz` is."""
    if pz.mates is None:
        raise AssertionError("pair_view takes zip_pairs' result; an interleaved parse goes to pairs_of")
    p1 = pz.mates[0]
    return Parsed(pz.dev, BorrowedBuffer(pz.codes), pz.n_bases, pz.n_records // 2, p1.rec_hdr,
                  np.ascontiguousarray(pz.rec_seq[0::2]), p1.names, p1.names_blob, p1.name_off, pz.n_masked)


def pairs_of(p: Parsed, *, check_names: bool = True) -> Parsed:
    """The pair view of an ordinary parse of an interleaved input (records 2i
    and 2i + 1 are the mates of pair i); `p` itself is the mate view.  No
    kernel runs.  An odd record count is refused, and with `check_names` the
    first pair whose two names differ (check_pair_names' rule).  Names and
    ``rec_hdr`` are mate 1's.  The view borrows p's codes: freeing it frees
    nothing."""
    R2 = int(p.n_records)
    if R2 % 2:
        raise AssertionError("%d records: an interleaved input holds the two mates of every pair, an even number"
                             % R2)
    if check_names:
        a, s, ln = _pair_keys(p)
        i = _first_name_mismatch((a, s[0::2], ln[0::2]), (a, s[1::2], ln[1::2]))
        if i >= 0:
            raise AssertionError("pair %d: the mates' names differ, %r and %r (a trailing /1 or /2 is ignored): the "
                                 "input is not interleaved" % (i + 1, bytes(p.names[2 * i]), bytes(p.names[2 * i + 1])))
    names, blob, name_off = _even_names(p)
    return Parsed(p.dev, BorrowedBuffer(p.codes), p.n_bases, R2 // 2, np.ascontiguousarray(p.rec_hdr[0::2]),
                  np.ascontiguousarray(p.rec_seq[0::2]), names, blob, name_off, p.n_masked)


def screen_pairs(pm: Parsed, pv: Parsed, table: CountResult, canonical: bool = False, *, median: bool = False,
                 min_count: Optional[int] = None, index: Optional[DeviceBuffer] = None,
                 index_bits: Optional[int] = None):
    """(stats, median or None, runs or None) of read pairs: `pm` the mate view
    and `pv` the pair view of the same codes.  stats: screen()'s rows per pair,
    joint over both mates' windows; median (`median`): record_quantile's lower
    median of the union of both mates' window counts, per pair; runs
    (`min_count`): record_runs' rows per MATE, 2R of them.  kman_window_counts
    runs once and serves both; the runs are taken first because the quantile
    leaves the words as scratch.  Each k-mer is looked up once per kernel."""
    _check_key_k(table.k, "screen")
    if pm.codes.ptr != pv.codes.ptr or pm.n_records != 2 * pv.n_records:
        raise AssertionError("screen_pairs: the two views are not of the same codes")
    if min_count is not None:
        min_count = _check_min_count(min_count)
    bits = _index_bits(table, index_bits)
    with pm.dev.scratch() as s:
        index = _index(s, table, index, bits)
        stats = screen(pv, table, canonical, index=index, index_bits=bits)
        med = runs = None
        if median or min_count is not None:
            d_wc = s.own(window_counts(pm, table, canonical, index=index, index_bits=bits))
            if min_count is not None:
                runs = record_runs(pm, d_wc, min_count)
            if median:
                med = record_quantile(pv, d_wc)
        return stats, med, runs


def pair_min_span(span):
    """The mates' spans (2R rows, solid_spans of the mate view) as one span
    per pair for screen_keep's ``min_solid_len``: (0, the shorter of the two
    stretches), so a pair passes when both stretches do."""
    start, end = (np.asarray(a, dtype=np.uint64).reshape(-1) for a in span)
    ln = end - np.minimum(start, end)
    m = np.minimum(ln[0::2], ln[1::2])
    return np.zeros(len(m), np.uint64), np.ascontiguousarray(m)


def emit_screen_pairs(pv: Parsed, stats: np.ndarray, keep, sink=None, median=None, *, span=None):
    """The `kmer screen` text of read pairs: emit_screen's lines with one line
    per pair of the pair view `pv` (the name is mate 1's); with `span` (the
    mates' solid_spans, 2R rows) four last columns "<TAB>START<TAB>END<TAB>
    START2<TAB>END2", mate 1's stretch and mate 2's (kman_format_screen_pair).
    Returned, or written to the binary file `sink`."""
    if span is None:
        return emit_screen(pv, stats, keep, sink, median=median)
    stats = np.asarray(stats, dtype=np.uint64).reshape(-1, 3)
    R = stats.shape[0]
    if R != pv.n_records:
        raise AssertionError("%d rows for %d pairs" % (R, pv.n_records))
    planes = np.ascontiguousarray(stats.T)
    off = np.ascontiguousarray(pv.name_off, dtype=np.uint64)
    keep = _keep_array(keep, R)
    kp = keep.ctypes.data_as(c_void_p) if keep is not None else None
    mp = None
    if median is not None:
        median = np.ascontiguousarray(median, dtype=np.uint32)
        if median.shape != (R,):
            raise AssertionError("median array of %r for %d pairs" % (median.shape, R))
        mp = median.ctypes.data_as(c_void_p)
    start, end = _span_arrays(span, 2 * R)
    return _to(sink, _format(N.lib().kman_format_screen_pair, planes.ctypes.data_as(c_void_p), mp,
                             start.ctypes.data_as(c_void_p), end.ctypes.data_as(c_void_p), R, kp, pv.names_blob,
                             off.ctypes.data_as(c_void_p)))


def emit_pair_reads(pm: Parsed, keep, sink1, sink2=None, *, span=None, trim=False):
    """`--reads-out` for read pairs: the listed pairs' records, both mates of a
    pair or neither.  `pm` is the mate view: zip_pairs' result (the mates'
    texts are cut into `sink1` and `sink2`, both calls of cut_records with the
    same keep array, so record i of one file and record i of the other are
    mates), or an interleaved parse (one interleaved text into `sink1`, the
    pair's flag applied to both of its records).  Under `trim` (`span`: the
    mates' solid_spans, 2R rows) each mate is cut to its own stretch and a pair
    with a mate that has no stretch is left out whole."""
    R = int(pm.n_records) // 2
    keep = _keep_array(keep, R)
    keep = np.ones(R, np.uint8) if keep is None else keep.copy()
    if trim:
        if span is None:
            raise AssertionError("trim needs the span arrays")
        start, end = _span_arrays(span, 2 * R)
        has = end > start
        keep[~(has[0::2] & has[1::2])] = 0
    if pm.mates is None:
        if sink2 is not None:
            raise AssertionError("an interleaved input is written to one file")
        return emit_reads(pm, np.repeat(keep, 2), sink1, span=(start, end) if trim else None, trim=trim)
    if sink2 is None:
        raise AssertionError("two inputs are written to two files")
    for m, sink, sl in ((pm.mates[0], sink1, slice(0, None, 2)), (pm.mates[1], sink2, slice(1, None, 2))):
        sp = (np.ascontiguousarray(start[sl]), np.ascontiguousarray(end[sl])) if trim else None
        emit_reads(m, keep, sink, span=sp, trim=trim)
