"""Coloured tables: reads among references (classify) and all pairs of inputs (compare)."""

from __future__ import annotations

import math
from ctypes import c_void_p
from typing import Optional

import numpy as np

from .. import _native as N
from .device import Device, DeviceBuffer
from .parsed import Parsed, _rec_seq
from .lookup import _keep_array
from .kmers import CountResult
from .join import free_result
from .output import _format, _to
from .tables import _check_key_k, _index, _index_bits, set_op


MAX_COLORS = N.KMAN_CLASSIFY_MAX_COLORS
UNASSIGNED, AMBIGUOUS = -1, -2  # classify_assign's values below the colours


def color_table(dev: Device, tables) -> CountResult:
    """The coloured table of 1..64 key-sorted distinct count tables of one k
    (join_groups(.., "count")): the union of their keys with count_bytes == 8,
    the "count" of a row being the mask of the tables that hold its key, bit c
    for tables[c].  The tables are CONSUMED: each one's buffers are freed as
    soon as it is folded in, so the peak is the union so far plus one table
    (free_result on them afterwards is harmless).  An empty table is legal:
    its colour is never hit.
    Table c's counts become 8-byte words all equal to 1 << c (kman_memset,
    kman_or_u64) and the table is folded into the running union with
    set_op(.., "union", "sum"): the bits are disjoint, so the sum is the OR,
    it never carries (KMAN_MATCH_ANY_SUM saturates only on a carry) and a mask
    with bit 63 set is inside filter_counts' unsigned range [1, 2^64 - 1]."""
    tables = list(tables)
    if not 1 <= len(tables) <= MAX_COLORS:
        raise AssertionError("a coloured table takes 1 to %d tables, got %d" % (MAX_COLORS, len(tables)))
    k = tables[0].k
    _check_key_k(k, "a coloured table")
    for t in tables:
        if t.k != k:
            raise AssertionError("the tables hold k-mers of different k: %d and %d" % (k, t.k))
    acc = None
    try:
        for c, t in enumerate(tables):
            m = dev.alloc(8 * max(t.n, 1))
            try:
                if t.n:
                    dev.memset(m, 0, 8 * t.n)
                    N.check(dev.ctx, N.lib().kman_or_u64(dev.ctx, c_void_p(m.ptr), t.n, 1 << c), "kman_or_u64")
            except BaseException:
                m.free()
                raise
            t.counts.free()
            # the table's keys move to the coloured rows: a new handle owns the allocation, the table's is emptied
            ukeys = object.__new__(DeviceBuffer)
            ukeys.dev, ukeys.ptr, ukeys.nbytes = t.ukeys.dev, t.ukeys.ptr, t.ukeys.nbytes
            t.ukeys.ptr = None
            col = CountResult(ukeys, m, 8, t.n, k)
            t.n = 0
            if acc is None:
                acc = col
                continue
            try:
                u = set_op(dev, acc, col, "union", "sum")
            finally:
                free_result(col)
            free_result(acc)
            acc = u
        res, acc = acc, None
        return res
    finally:
        free_result(acc)


def classify(p: Parsed, ctable: CountResult, n_colors: int, canonical: bool = False, specific: bool = False,
             index: Optional[DeviceBuffer] = None, index_bits: Optional[int] = None, planes: bool = False):
    """kman_classify_records + kman_classify_pick: for every record of p,
    (windows, best, hits, second), four u32 arrays of n_records: its valid
    k-mer windows, the lowest-indexed reference with the most hits
    (N.KMAN_CLASSIFY_NONE when nothing hit), those hits, and the most hits
    among the other references.  `ctable`: color_table()'s result for
    n_colors references, k = ctable.k.  specific: a window counts only for the
    one reference that holds its k-mer.  canonical, index, index_bits as for
    screen().  planes: a fifth result, the (n_records, n_colors) u32 hits of
    every reference; without it only the windows plane and the three picked
    planes leave the device."""
    _check_key_k(ctable.k, "classify")
    if isinstance(n_colors, bool) or not isinstance(n_colors, (int, np.integer)) or not 1 <= n_colors <= MAX_COLORS:
        raise AssertionError("n_colors must be an integer in [1, %d], got %r" % (MAX_COLORS, n_colors))
    if ctable.count_bytes != 8:
        raise AssertionError("classify takes a coloured table (8-byte masks: color_table), got %d-byte counts"
                             % ctable.count_bytes)
    dev, k, R, nc = p.dev, ctable.k, int(p.n_records), int(n_colors)
    bits = _index_bits(ctable, index_bits)
    rec_seq = np.asarray(p.rec_seq, dtype=np.uint64)
    if R:
        ends = np.concatenate([rec_seq[1:], np.asarray([p.n_bases], dtype=np.uint64)])
        if int((ends - np.minimum(rec_seq, ends)).max()) >= 1 << 32:
            raise AssertionError("classify counts in 32 bits: a record of 2^32 or more bases is refused")
    if R == 0:
        z = np.zeros(0, np.uint32)
        return (z, z.copy(), z.copy(), z.copy()) + ((np.zeros((0, nc), np.uint32),) if planes else ())
    flags = (N.KMAN_CANONICAL if canonical else 0) | (N.KMAN_CLASSIFY_SPECIFIC if specific else 0)
    with dev.scratch() as s:
        index = _index(s, ctable, index, bits)
        d_rec, _ = _rec_seq(s, p)
        d_out = s.alloc(4 * (1 + nc) * R)
        d_pick = s.alloc(12 * R)
        N.check(dev.ctx, N.lib().kman_classify_records(
            dev.ctx, c_void_p(p.codes.ptr), p.n_bases, k, flags, c_void_p(d_rec.ptr), R, c_void_p(ctable.ukeys.ptr),
            c_void_p(ctable.counts.ptr), ctable.n, c_void_p(index.ptr), bits, nc, c_void_p(d_out.ptr)),
            "kman_classify_records")
        N.check(dev.ctx, N.lib().kman_classify_pick(dev.ctx, c_void_p(d_out.ptr), R, nc, c_void_p(d_pick.ptr)),
                "kman_classify_pick")
        windows = dev.download(d_out, R, np.uint32)
        pick = dev.download(d_pick, 3 * R, np.uint32).reshape(3, R)
        res = (windows, pick[0].copy(), pick[1].copy(), pick[2].copy())
        if planes:
            res += (np.ascontiguousarray(dev.download(d_out, nc * R, np.uint32, 4 * R).reshape(nc, R).T),)
        return res


def classify_assign(windows, best, hits, second, min_hits: int = 1, min_frac: float = 0.0,
                    min_margin: int = 1) -> np.ndarray:
    """The reference each record of classify()'s arrays is assigned to, an
    int32 array: UNASSIGNED (-1) when hits < max(min_hits, 1) or hits <
    min_frac * windows (float64), else AMBIGUOUS (-2) when hits - second <
    min_margin, else `best`.  min_margin >= 1: a tie is never decided by the
    order of the references."""
    for name, v in (("min_hits", min_hits), ("min_margin", min_margin)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
            raise AssertionError("%s must be an integer, got %r" % (name, v))
    if min_hits < 0:
        raise AssertionError("min_hits must be >= 0, got %d" % min_hits)
    if min_margin < 1:
        raise AssertionError("min_margin must be >= 1, got %d" % min_margin)
    if isinstance(min_frac, bool) or not isinstance(min_frac, (int, float, np.integer, np.floating)) or \
            not 0.0 <= min_frac <= 1.0:  # (a NaN is refused too)
        raise AssertionError("min_frac must be in [0, 1], got %r" % (min_frac,))
    w, b, h, s = (np.asarray(a, dtype=np.uint32).reshape(-1) for a in (windows, best, hits, second))
    if not (w.shape == b.shape == h.shape == s.shape):
        raise AssertionError("classify_assign: arrays of %r, %r, %r and %r" % (w.shape, b.shape, h.shape, s.shape))
    hf, h64 = h.astype(np.float64), h.astype(np.int64)
    un = (h64 < max(int(min_hits), 1)) | (hf < float(min_frac) * w.astype(np.float64)) | \
        (b == np.uint32(N.KMAN_CLASSIFY_NONE))
    amb = (h64 - s.astype(np.int64)) < int(min_margin)
    out = np.where(un, UNASSIGNED, np.where(amb, AMBIGUOUS, b.astype(np.int64)))
    return out.astype(np.int32)


def _label_blob(labels):
    labels = [x if isinstance(x, bytes) else str(x).encode("utf-8", errors="surrogateescape") for x in labels]
    if not 1 <= len(labels) <= MAX_COLORS:
        raise AssertionError("1 to %d labels, got %d" % (MAX_COLORS, len(labels)))
    off = np.zeros(len(labels) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(x) for x in labels])
    return b"".join(labels), off


def emit_classify(p: Parsed, labels, windows, assign, hits, second, sink=None, *, planes=None, keep=None):
    """The `kmer classify` text: one "name<TAB>windows<TAB>LABEL<TAB>hits<TAB>
    second" line per record with keep != 0 (None: all), in input order
    (kman_format_classify); LABEL is labels[assign], "?" for AMBIGUOUS, "-" for
    UNASSIGNED.  `planes` (classify(.., planes=True)'s (n_records, n_colors)
    array) appends one column per reference.  Returned, or written to the
    binary file `sink`."""
    R = int(p.n_records)
    blob, loff = _label_blob(labels)
    nc = len(loff) - 1
    w, h, s = (np.ascontiguousarray(a, dtype=np.uint32).reshape(-1) for a in (windows, hits, second))
    a = np.ascontiguousarray(assign, dtype=np.int32).reshape(-1)
    for x in (w, h, s, a):
        if x.shape != (R,):
            raise AssertionError("array of %r for %d records" % (x.shape, R))
    if R and int(a.max()) >= nc:
        raise AssertionError("assignment %d with %d labels" % (int(a.max()), nc))
    pp = None
    if planes is not None:
        planes = np.asarray(planes, dtype=np.uint32)
        if planes.shape != (R, nc):
            raise AssertionError("hit planes of %r for %d records and %d labels" % (planes.shape, R, nc))
        planes = np.ascontiguousarray(planes.T)
        pp = planes.ctypes.data_as(c_void_p)
    keep = _keep_array(keep, R)
    kp = keep.ctypes.data_as(c_void_p) if keep is not None else None
    off = np.ascontiguousarray(p.name_off, dtype=np.uint64)
    return _to(sink, _format(N.lib().kman_format_classify, w.ctypes.data_as(c_void_p), a.ctypes.data_as(c_void_p),
                             h.ctypes.data_as(c_void_p), s.ctypes.data_as(c_void_p), pp, nc, R, kp, blob,
                             loff.ctypes.data_as(c_void_p), p.names_blob, off.ctypes.data_as(c_void_p)))


# ------------------------------------------------- all pairs of a coloured table (compare)

COMPARE_METRICS = ("jaccard", "dist", "shared", "containment")


def mask_gram(dev: Device, ctable: CountResult, n_colors: int):
    """kman_mask_gram on a coloured table (color_table): (gram, occ, private),
    numpy u64 arrays of shapes (n_colors, n_colors), (n_colors + 1,) and
    (n_colors,).  gram[i][j]: the rows held by references i and j (the
    diagonal: each reference's rows); occ[p]: the rows held by exactly p
    references; private[c]: the rows held by reference c alone.  An empty
    table gives zeros."""
    if isinstance(n_colors, bool) or not isinstance(n_colors, (int, np.integer)) or not 1 <= n_colors <= MAX_COLORS:
        raise AssertionError("n_colors must be an integer in [1, %d], got %r" % (MAX_COLORS, n_colors))
    if ctable.count_bytes != 8:
        raise AssertionError("mask_gram takes a coloured table (8-byte masks: color_table), got %d-byte counts"
                             % ctable.count_bytes)
    nc, n = int(n_colors), int(ctable.n)
    words = nc * nc + (nc + 1) + nc
    with dev.scratch() as s:
        d_out = s.alloc(8 * words)
        N.check(dev.ctx, N.lib().kman_mask_gram(
            dev.ctx, c_void_p(ctable.counts.ptr if n else None), n, nc, c_void_p(d_out.ptr),
            c_void_p(d_out.ptr + 8 * nc * nc), c_void_p(d_out.ptr + 8 * (nc * nc + nc + 1))), "kman_mask_gram")
        out = dev.download(d_out, words, np.uint64)
    return out[:nc * nc].reshape(nc, nc).copy(), out[nc * nc:nc * nc + nc + 1].copy(), out[nc * nc + nc + 1:].copy()


def compare_rows(gram, k: int):
    """The per-pair metrics of mask_gram's matrix, computed in float64 from
    the exact integers: a list of (i, j, a, b, s, jaccard, cont_i, cont_j,
    dist) for every pair i < j, a = gram[i][i], b = gram[j][j], s =
    gram[i][j] as Python ints.  See compare_metrics."""
    g = np.asarray(gram, dtype=np.uint64)
    if g.ndim != 2 or g.shape[0] != g.shape[1]:
        raise AssertionError("compare_rows takes a square matrix, got %r" % (g.shape,))
    rows = []
    for i in range(g.shape[0]):
        for j in range(i + 1, g.shape[0]):
            a, b, s = int(g[i, i]), int(g[j, j]), int(g[i, j])
            rows.append((i, j, a, b, s) + compare_metrics(a, b, s, k))
    return rows


def compare_metrics(a: int, b: int, s: int, k: int):
    """(jaccard, containment of the first, containment of the second, Mash
    distance) of two k-mer sets of a and b k-mers that share s, with u = a +
    b - s: J = s / u (0 when u == 0); s / a and s / b (0 for an empty set);
    D = -ln(2 J / (1 + J)) / k, 1 when J == 0, exactly 0 when J == 1, clamped
    to [0, 1]."""
    if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or k < 1:
        raise AssertionError("k must be a positive integer, got %r" % (k,))
    a, b, s = int(a), int(b), int(s)
    u = a + b - s
    jac = float(s) / float(u) if u else 0.0
    ca = float(s) / float(a) if a else 0.0
    cb = float(s) / float(b) if b else 0.0
    if jac <= 0.0:
        dist = 1.0
    elif jac >= 1.0:
        dist = 0.0
    else:
        dist = min(1.0, max(0.0, -math.log(2.0 * jac / (1.0 + jac)) / float(k)))
    return jac, ca, cb, dist


def _compare_labels(labels, n: int):
    labels = [x.decode("utf-8", errors="surrogateescape") if isinstance(x, bytes) else str(x) for x in labels]
    if len(labels) != n:
        raise AssertionError("%d labels for %d inputs" % (len(labels), n))
    return labels


def emit_compare(labels, gram, k: int, sink=None):
    """The `kmer compare` text: one "LABEL_I<TAB>LABEL_J<TAB>KMERS_I<TAB>
    KMERS_J<TAB>SHARED<TAB>JACCARD<TAB>CONT_I<TAB>CONT_J<TAB>DIST" line per
    pair i < j in input order, the reals as %.6f.  Plain host formatting.
    Returned, or written to the binary file `sink`."""
    g = np.asarray(gram, dtype=np.uint64)
    labels = _compare_labels(labels, g.shape[0])
    out = ["%s\t%s\t%d\t%d\t%d\t%.6f\t%.6f\t%.6f\t%.6f\n" % ((labels[i], labels[j]) + tuple(r))
           for (i, j, *r) in compare_rows(g, k)]
    return _to(sink, "".join(out).encode("utf-8", errors="surrogateescape"))


def emit_compare_matrix(labels, gram, k: int, metric: str = "dist", sink=None):
    """The `kmer compare --matrix` text: a first line with the number of
    inputs, then "LABEL<TAB>v_0<TAB>...<TAB>v_{n-1}" per input.  metric:
    "dist", "jaccard", "containment" (row in column, gram[r][c] / gram[r][r]:
    not symmetric) as %.6f, or "shared" as integers.  The diagonal is the
    input's k-mers (shared), 1 (jaccard, containment; 0 for an empty input)
    and 0 (dist)."""
    if metric not in COMPARE_METRICS:
        raise AssertionError("metric must be one of %s, got %r" % (", ".join(COMPARE_METRICS), metric))
    g = np.asarray(gram, dtype=np.uint64)
    n = g.shape[0]
    labels = _compare_labels(labels, n)
    out = ["%d\n" % n]
    for r in range(n):
        cells = []
        for c in range(n):
            a, b, s = int(g[r, r]), int(g[c, c]), int(g[r, c])
            if metric == "shared":
                cells.append("%d" % s)
                continue
            jac, ca, _, dist = compare_metrics(a, b, s, k)
            if r == c:
                jac, ca, dist = (1.0 if a else 0.0), (1.0 if a else 0.0), 0.0
            cells.append("%.6f" % {"jaccard": jac, "containment": ca, "dist": dist}[metric])
        out.append("\t".join([labels[r]] + cells) + "\n")
    return _to(sink, "".join(out).encode("utf-8", errors="surrogateescape"))


def emit_occupancy(occ, sink=None):
    """The `kmer compare --occupancy` text, the pan-genome spectrum: "P<TAB>
    KMERS" for P = 1 .. n, the k-mers held by exactly P inputs (P = n: the
    core).  `occ`: mask_gram's second array (occ[0] is not written)."""
    o = np.asarray(occ, dtype=np.uint64).reshape(-1)
    return _to(sink, "".join("%d\t%d\n" % (p, int(o[p])) for p in range(1, len(o))).encode())


def emit_compare_summary(labels, gram, private, sink=None):
    """The `kmer compare --summary` text: "LABEL<TAB>KMERS<TAB>PRIVATE" per
    input (its k-mers, and those of them no other input holds)."""
    g = np.asarray(gram, dtype=np.uint64)
    pr = np.asarray(private, dtype=np.uint64).reshape(-1)
    labels = _compare_labels(labels, g.shape[0])
    if len(pr) != len(labels):
        raise AssertionError("%d private counts for %d inputs" % (len(pr), len(labels)))
    out = ["%s\t%d\t%d\n" % (lab, int(g[c, c]), int(pr[c])) for c, lab in enumerate(labels)]
    return _to(sink, "".join(out).encode("utf-8", errors="surrogateescape"))
