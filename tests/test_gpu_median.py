"""Per-read median k-mer abundance on the GPU: kman_window_counts against the
plain-Python statement (tests/median_cases.py) and against
kman_screen_records' planes, kman_record_quantile on hand-built words against
numpy.sort, engine.screen_median and `kmer screen --median` against the
statement, all for equality."""

from __future__ import annotations

import gzip
from ctypes import byref, c_uint64, c_void_p

import numpy as np
import pytest
from click.testing import CliRunner

import median_cases as mc
import screen_cases as sc

pytestmark = pytest.mark.gpu

from kman_amd import _native as N  # noqa: E402

T = N.KMAN_SCREEN_TILE
CAP = N.KMAN_SCREEN_REC_CAP
C = N.KMAN_QUANTILE_REC_CAP
Q = N.KMAN_QUANTILE_TILE
S = N.KMAN_QUANTILE_SLICE
NONE = N.KMAN_WC_NONE
SAT = mc.SAT
PAD = 16  # sentinel words after an output
SENT32 = 0xA5A5A5A5
SENT64 = 0xA5A5A5A5A5A5A5A5


@pytest.fixture(scope="module")
def dev():
    from kman_amd import engine

    return engine.default_device()


def _up(dev, arr):
    arr = np.ascontiguousarray(arr)
    buf = dev.alloc(max(16, arr.nbytes))
    if arr.nbytes:
        dev.upload(buf, arr)
    return buf


# ---------------------------------------------------------- kman_window_counts


def _tables(dev, records, k, table, cb, bits):
    from kman_amd import engine

    codes, rec_seq, n_bases = sc.codes_of(records)
    keys, counts = sc.table_rows(table, cb)
    if bits is None:
        bits = engine.default_index_bits(len(keys), k)
    bufs = [_up(dev, codes), _up(dev, rec_seq), _up(dev, keys), _up(dev, counts), dev.alloc(8 * ((1 << bits) + 1))]
    assert N.lib().kman_table_index(dev.ctx, c_void_p(bufs[2].ptr), len(keys), k, bits, c_void_p(bufs[4].ptr)) == N.KMAN_OK
    return bufs, rec_seq, n_bases, len(keys), bits


def _window_counts(dev, records, k, table, canonical=False, cb=4, bits=None, with_screen=False):
    """kman_window_counts on the helper's device layout of `records`, the
    output pre-filled with a pattern; the n_bases words (and, with_screen,
    kman_screen_records' (n_records, 3) rows on the same buffers)."""
    bufs, rec_seq, n_bases, nt, bits = _tables(dev, records, k, table, cb, bits)
    L = N.lib()
    flags = N.KMAN_CANONICAL if canonical else 0
    d_wc = _up(dev, np.full(n_bases + PAD, SENT32, np.uint32))
    bufs.append(d_wc)
    try:
        d_codes, d_rec, d_keys, d_counts, d_index = bufs[:5]
        rc = L.kman_window_counts(dev.ctx, c_void_p(d_codes.ptr), n_bases, k, flags, c_void_p(d_keys.ptr),
                                  c_void_p(d_counts.ptr), cb, nt, c_void_p(d_index.ptr), bits, c_void_p(d_wc.ptr))
        assert rc == N.KMAN_OK, L.kman_last_error(dev.ctx)
        got = dev.download(d_wc, n_bases + PAD, np.uint32)
        assert np.all(got[n_bases:] == SENT32)  # words past n_bases untouched
        st = None
        if with_screen:
            R = len(records)
            d_out = _up(dev, np.full(3 * R, SENT64, np.uint64))
            bufs.append(d_out)
            rc = L.kman_screen_records(dev.ctx, c_void_p(d_codes.ptr), n_bases, k, flags, c_void_p(d_rec.ptr), R,
                                       c_void_p(d_keys.ptr), c_void_p(d_counts.ptr), cb, nt, c_void_p(d_index.ptr),
                                       bits, c_void_p(d_out.ptr))
            assert rc == N.KMAN_OK
            st = np.ascontiguousarray(dev.download(d_out, 3 * R, np.uint64).reshape(3, R).T)
        return got[:n_bases], rec_seq, n_bases, st
    finally:
        for b in bufs:
            b.free()


_WANT = {}


def _want_words(records, k, table, canonical):
    """mc.window_words, computed once per (records, k, table, canonical)."""
    key = (tuple(records), k, canonical, tuple(sorted(table.items())))
    if key not in _WANT:
        _WANT[key] = np.asarray(mc.window_words(records, k, table, canonical), dtype=np.uint32)
    return _WANT[key]


def _check_wc(dev, records, k, table, canonical=False, cb=4, bits=None, consistent=True):
    want = _want_words(records, k, table, canonical)
    got, rec_seq, n_bases, st = _window_counts(dev, records, k, table, canonical, cb, bits, with_screen=True)
    assert n_bases == len(want)
    np.testing.assert_array_equal(got, want)
    # the same records through kman_screen_records: non-NONE words = windows,
    # nonzero ones = hits, their sum = the sum plane (when nothing saturates)
    ends = np.concatenate([rec_seq[1:], [n_bases]]).astype(np.int64)
    sat = max(table.values(), default=0) > SAT
    for r, (a, b) in enumerate(zip(rec_seq.astype(np.int64), ends)):
        w = got[a:b][got[a:b] != NONE].astype(np.uint64)
        assert len(w) == st[r, 0] and np.count_nonzero(w) == st[r, 1], r
        assert sat or int(w.sum()) == int(st[r, 2]), r
    med = mc.record_quantiles(got.tolist(), rec_seq, n_bases)
    if consistent and min(table.values(), default=1) >= 1:
        assert mc.property_holds(st, med)
    return got, st


def _half_table(records, k, canonical, seed=9):
    own = [r for r in records if len(r[1]) >= k][::2]
    return sc.table_of(own + sc.records_of([400, 300], seed, "x"), k, canonical)


LAYOUTS = sorted(sc.layouts(5, T, CAP))


@pytest.mark.parametrize("k", [5, 21])
@pytest.mark.parametrize("name", LAYOUTS)
def test_window_counts_record_layouts(dev, name, k):
    lengths = sc.layouts(k, T, CAP)[name]
    records = sc.records_of(lengths, seed=len(name) + k)
    for canonical, cb in ((False, 4), (True, 8)):
        got, st = _check_wc(dev, records, k, _half_table(records, k, canonical), canonical, cb)
        if max(lengths) >= k + 1:
            assert st[:, 1].sum() > 0
        if name in ("bases_k_minus_1", "two_short", "only_small"):
            assert np.all(got == NONE)  # (bases_k_minus_1: n_bases < k, nothing is launched)
    if name == "reads150":
        # the last k - 1 bases of every record hold NONE
        got, _ = _check_wc(dev, records, k, sc.table_of(records, k))
        assert np.all(got.reshape(-1)[150 - k + 1:150] == NONE) and np.all(got[:150 - k + 1] >= 1)


@pytest.mark.parametrize("k", [2, 5, 21, 32])
def test_window_counts_n_runs_and_keys(dev, k):
    records = sc.n_run_records(k, T) + sc.records_of([150] * 6 + [k, k + 1, 33], seed=k, prefix="read")
    if k == 32:
        records += [("polyA", "A" * 40), ("polyT", "T" * 40)]
    for canonical in (False, True):
        for cb in (4, 8):
            table = sc.table_of(records[:1] + records[4::2], k, canonical)
            got, st = _check_wc(dev, records, k, table, canonical, cb)
            assert np.count_nonzero(got == NONE) > k and (k < 21 or np.count_nonzero(got == 0) > 0)
        _check_wc(dev, records, k, {}, canonical)  # an empty table: every valid window is 0
        if not canonical:  # an explicit index width of 1 and of the maximum, next to the default
            for bits in (1, min(2 * k, N.KMAN_SCREEN_MAX_INDEX_BITS)):
                _check_wc(dev, records, k, sc.table_of(records[4:7], k), bits=bits)
    got, _ = _check_wc(dev, records, k, {})
    assert set(np.unique(got).tolist()) == {0, NONE}


def test_window_counts_saturate(dev):
    k = 7
    records = sc.records_of([200, 90], seed=4)
    ws = sorted(sc.table_of(records, k))
    big = [SAT - 1, SAT, SAT + 1, 1 << 32, 1 << 40]
    table = {w: big[i] if i < len(big) else 3 for i, w in enumerate(ws)}
    got, _ = _check_wc(dev, records, k, table, cb=8)
    assert np.count_nonzero(got == SAT) >= 4 and np.count_nonzero(got == SAT - 1) >= 1
    assert mc.SAT == 0xFFFFFFFE and not np.any((got == NONE) & (np.arange(len(got)) < 200 - k + 1))


def test_window_counts_refused(dev):
    records = sc.records_of([150] * 3, seed=2)
    bufs, rec_seq, n, nt, _ = _tables(dev, records, 9, sc.table_of(records, 9), 4, 4)
    fill = np.full(n + PAD, SENT32, np.uint32)
    d_wc = _up(dev, fill)
    L = N.lib()
    try:
        d_codes, _, d_keys, d_counts, d_index = bufs

        def call(k=9, flags=0, cb=4, bits=4, n_bases=n, wc=d_wc.ptr):
            return L.kman_window_counts(dev.ctx, c_void_p(d_codes.ptr), n_bases, k, flags, c_void_p(d_keys.ptr),
                                        c_void_p(d_counts.ptr), cb, nt, c_void_p(d_index.ptr), bits, c_void_p(wc))

        for kw in (dict(k=1), dict(k=33), dict(flags=N.KMAN_RC), dict(flags=N.KMAN_CANONICAL | N.KMAN_MIXED),
                   dict(cb=2), dict(cb=16), dict(bits=0), dict(bits=19), dict(bits=25), dict(wc=None),
                   dict(wc=d_wc.ptr + 4)):
            assert call(**kw) == N.KMAN_EINVAL, kw
        assert call(n_bases=0) == N.KMAN_OK
        np.testing.assert_array_equal(dev.download(d_wc, n + PAD, np.uint32), fill)  # nothing was written
        assert call(n_bases=8) == N.KMAN_OK  # fewer bases than k: every word is NONE
        got = dev.download(d_wc, n + PAD, np.uint32)
        assert np.all(got[:8] == NONE) and np.all(got[8:] == SENT32)
        assert call() == N.KMAN_OK  # the context is still usable
        want = mc.window_words(records, 9, sc.table_of(records, 9))
        np.testing.assert_array_equal(dev.download(d_wc, n, np.uint32), np.asarray(want, np.uint32))
    finally:
        for b in bufs + [d_wc]:
            b.free()


# -------------------------------------------------------- kman_record_quantile


def _plan(n_long, n_values):
    out = c_uint64(0)
    assert N.lib().kman_record_quantile_plan(n_long, n_values, byref(out)) == N.KMAN_OK
    return out.value


def _quantile(dev, words, rec_seq, n_bases, num=1, den=2, work_bytes=None, n_records=None, null=None):
    """One kman_record_quantile call on a fresh copy of `words`: (return code,
    the n_records words, the words after them)."""
    from kman_amd import engine

    words = np.ascontiguousarray(words, dtype=np.uint32)
    rec_seq = np.ascontiguousarray(rec_seq, dtype=np.uint64)
    R = len(rec_seq) if n_records is None else n_records
    plan = _plan(*engine.quantile_plan(rec_seq, n_bases))
    if work_bytes is None:
        work_bytes = plan
    bufs = [_up(dev, words), _up(dev, rec_seq), dev.alloc(max(16, plan)),
            _up(dev, np.full(len(rec_seq) + PAD, SENT32, np.uint32))]
    try:
        ptrs = [b.ptr for b in bufs]
        if null is not None:
            ptrs[null] = None
        rc = N.lib().kman_record_quantile(dev.ctx, c_void_p(ptrs[0]), n_bases, c_void_p(ptrs[1]), R, num, den,
                                          c_void_p(ptrs[2]), work_bytes, c_void_p(ptrs[3]))
        got = dev.download(bufs[3], len(rec_seq) + PAD, np.uint32)
        return rc, got[:len(rec_seq)], got[len(rec_seq):]
    finally:
        for b in bufs:
            b.free()


def _numpy_quantiles(words, rec_seq, n_bases, num, den):
    rs = np.minimum(np.asarray(rec_seq, dtype=np.uint64), np.uint64(n_bases)).astype(np.int64)
    ends = np.concatenate([rs[1:], [n_bases]])
    out = np.zeros(len(rs), np.uint32)
    for r, (a, b) in enumerate(zip(rs, ends)):
        v = np.sort(words[a:max(a, b)][words[a:max(a, b)] != NONE])
        if len(v):
            out[r] = v[(len(v) - 1) * num // den]
    return out


FRACTIONS = [(0, 1), (1, 2), (1, 1), (1, 4), (3, 4), (99, 100), (65535, 65535)]

RECORD_LAYOUTS = {
    # name: (bases before the first record, record lengths)
    "edges": (0, [0, 1, 2, C - 1, C, C + 1, 0, 5, 150, 3]),
    "chunk_edges": (0, [C, C - 101, 100, 1, 300, C - 300, C, 150, 37]),   # starts at Q - 1, Q and 2 Q; ends at Q
    "cross_chunk": (7, [C - 8, C, C, 9, 60, 11]),                         # a record of C bases from base Q - 1
    "small_runs": (0, [150] + [1, 0] * (S + 10) + [150, 21]),             # > S records start in chunk 0
    "small_runs_carry": (0, [C, C - 10, 150] + [1, 0] * (S + 10) + [150]),  # > S in chunk 1, after a carried-in record
    "only_empty": (0, [0] * 50),
    "empty_after_bases": (40, [0] * 5),
    "one_long_spanning": (3, [10, 3 * Q + 500, 20]),                      # one long record over more than 3 chunks
    "three_long": (0, [C + 1, 100, 0, 2 * C, 50, 7, C + 700, 12]),        # short records between long ones
    "long_first_and_last": (0, [C + 5, 10, 0, C + 9]),
    "end_at_chunk": (0, [C, C, C - 5, 5, C, 0]),                          # n_bases = 2 Q: an empty record starts there
}


def _layout(name):
    lead, lengths = RECORD_LAYOUTS[name]
    rec_seq = lead + np.concatenate([[0], np.cumsum(lengths)[:-1]]).astype(np.uint64)
    return rec_seq.astype(np.uint64), lead + int(sum(lengths))


def _values(kind, n, seed):
    rng = np.random.default_rng(seed)
    if kind == "random":  # few distinct values (heavy duplicates around every rank), a fifth NONE
        v = rng.choice(np.asarray([0, 1, 2, 3, 7, 255, 256, 65536, 1 << 24, SAT, 77777], np.uint32), n)
        v[rng.random(n) < 0.2] = NONE
    elif kind == "wide":  # every byte of the word matters
        v = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    elif kind == "equal":
        v = np.full(n, 41, np.uint32)
    elif kind == "descending":
        v = (np.uint32(SAT) - np.arange(n, dtype=np.uint32))
    elif kind == "none":
        v = np.full(n, NONE, np.uint32)
    elif kind == "interleaved":
        v = rng.integers(0, 1000, n, dtype=np.uint64).astype(np.uint32)
        v[::2] = NONE
    elif kind == "extremes":
        v = np.where(rng.random(n) < 0.5, np.uint32(0), np.uint32(SAT)).astype(np.uint32)
    else:
        raise KeyError(kind)
    return np.ascontiguousarray(v, dtype=np.uint32)


@pytest.mark.parametrize("name", sorted(RECORD_LAYOUTS))
def test_record_quantile_layouts(dev, name):
    from kman_amd import engine

    rec_seq, n_bases = _layout(name)
    n_long = engine.quantile_plan(rec_seq, n_bases)[0]
    assert n_long == {"edges": 1, "one_long_spanning": 1, "three_long": 3, "long_first_and_last": 2}.get(name, 0)
    if name.startswith("small_runs"):
        per_chunk = np.bincount((rec_seq // Q).astype(np.int64))
        assert per_chunk.max() > S and (name == "small_runs") == (per_chunk[0] > S)
    if name == "chunk_edges":
        assert {Q - 101, Q - 1, Q, 2 * Q} <= set(rec_seq.tolist())
    if name == "cross_chunk":
        assert Q - 1 in set(rec_seq.tolist())
    if name == "end_at_chunk":
        assert n_bases == 2 * Q == int(rec_seq[-1])
    for kind in ("random", "wide"):
        words = _values(kind, n_bases, len(name))
        for num, den in FRACTIONS:
            rc, got, tail = _quantile(dev, words, rec_seq, n_bases, num, den)
            assert rc == N.KMAN_OK, (kind, num, den, N.lib().kman_last_error(dev.ctx))
            np.testing.assert_array_equal(got, _numpy_quantiles(words, rec_seq, n_bases, num, den),
                                          err_msg="%s %s %d/%d" % (name, kind, num, den))
            assert np.all(tail == SENT32)
    words = _values("random", n_bases, 5)
    assert _numpy_quantiles(words, rec_seq, n_bases, 1, 2).tolist() == mc.record_quantiles(words.tolist(), rec_seq,
                                                                                           n_bases)
    a, b = (_quantile(dev, words, rec_seq, n_bases, 1, 2)[1] for _ in range(2))
    assert a.tobytes() == b.tobytes()  # the same call on a fresh copy: identical bytes


@pytest.mark.parametrize("kind", ["equal", "descending", "none", "interleaved", "extremes"])
def test_record_quantile_values(dev, kind):
    for name in ("edges", "three_long", "cross_chunk"):
        rec_seq, n_bases = _layout(name)
        words = _values(kind, n_bases, 3)
        for num, den in FRACTIONS:
            rc, got, tail = _quantile(dev, words, rec_seq, n_bases, num, den)
            assert rc == N.KMAN_OK
            want = _numpy_quantiles(words, rec_seq, n_bases, num, den)
            np.testing.assert_array_equal(got, want, err_msg="%s %s %d/%d" % (name, kind, num, den))
            assert np.all(tail == SENT32)
        if kind == "none":
            assert not want.any()  # a long record that is all NONE included
        if kind == "extremes" and name == "three_long":
            assert {0, SAT} <= set(want.tolist())


def test_record_quantile_one_long_record_all_none(dev):
    rec_seq, n_bases = _layout("three_long")
    words = _values("random", n_bases, 8)
    words[int(rec_seq[3]):int(rec_seq[4])] = NONE
    rc, got, _ = _quantile(dev, words, rec_seq, n_bases)
    assert rc == N.KMAN_OK and got[3] == 0 and got[0] > 0
    np.testing.assert_array_equal(got, _numpy_quantiles(words, rec_seq, n_bases, 1, 2))


def test_record_quantile_work_buffer_and_refusals(dev):
    from kman_amd import engine

    rec_seq, n_bases = _layout("three_long")
    words = _values("random", n_bases, 6)
    want = _numpy_quantiles(words, rec_seq, n_bases, 1, 2)
    plan = _plan(*engine.quantile_plan(rec_seq, n_bases))
    assert plan > _plan(0, 0)
    for wb in (plan - 1, _plan(0, 0), _plan(0, 0) - 1, 0):  # one byte short; the short records' size; less
        rc, got, tail = _quantile(dev, words, rec_seq, n_bases, work_bytes=wb)
        assert rc == N.KMAN_ECAP and np.all(tail == SENT32), wb
    rc, got, _ = _quantile(dev, words, rec_seq, n_bases)  # the context is still usable
    assert rc == N.KMAN_OK
    np.testing.assert_array_equal(got, want)
    # only short records: the plan of (0, 0) is accepted, one byte less is not
    rs, nb = _layout("chunk_edges")
    w2 = _values("random", nb, 7)
    rc, got, _ = _quantile(dev, w2, rs, nb, work_bytes=_plan(0, 0))
    assert rc == N.KMAN_OK
    np.testing.assert_array_equal(got, _numpy_quantiles(w2, rs, nb, 1, 2))
    # refused arguments leave d_q as it was
    for kw in (dict(den=0), dict(num=2, den=1), dict(num=3, den=65536), dict(den=65536), dict(null=0), dict(null=1),
               dict(null=2), dict(null=3)):
        rc, got, tail = _quantile(dev, words, rec_seq, n_bases, **kw)
        assert rc == N.KMAN_EINVAL, kw
        assert np.all(got == SENT32) and np.all(tail == SENT32), kw
    rc, got, tail = _quantile(dev, words, rec_seq, n_bases, n_records=0)  # no record: nothing is done
    assert rc == N.KMAN_OK and np.all(got == SENT32) and np.all(tail == SENT32)
    rc, got, _ = _quantile(dev, words, rec_seq, n_bases, 65535, 65535)
    assert rc == N.KMAN_OK
    np.testing.assert_array_equal(got, _numpy_quantiles(words, rec_seq, n_bases, 1, 1))


def test_record_quantile_clamps_entries(dev):
    """Entries past n_bases are clamped: the records there are empty."""
    rec_seq = np.asarray([0, 100, 250, 400, 900], dtype=np.uint64)
    words = _values("wide", 300, 2)
    rc, got, tail = _quantile(dev, words, rec_seq, 300)
    assert rc == N.KMAN_OK and np.all(tail == SENT32)
    np.testing.assert_array_equal(got, _numpy_quantiles(words, rec_seq, 300, 1, 2))
    assert got[3] == 0 and got[4] == 0


# ------------------------------------------------------------------ engine API


def _engine_median(dev, reads_text, table_text, k, canonical=False, fmt="auto", min_qual=0, index_bits=None,
                   min_count=1):
    from kman_amd import engine

    p = engine.parse(dev, table_text)
    try:
        table = engine.join_groups(p, k, False, "count", canonical=canonical)
    finally:
        p.free()
    if table is None:
        table = engine.empty_count(dev, k)
    elif min_count > 1:
        solid = engine.filtered_copy(dev, table, min_count, None)
        engine.free_result(table)
        table = solid
    p = engine.parse(dev, reads_text, fmt, min_qual)
    try:
        st, med = engine.screen_median(p, table, canonical, index_bits=index_bits)
        assert st.shape == (p.n_records, 3) and med.shape == (p.n_records,) and med.dtype == np.uint32
        np.testing.assert_array_equal(st, engine.screen(p, table, canonical, index_bits=index_bits))
        idx = engine.table_index(dev, table, index_bits)
        try:
            st2, mx = engine.screen_median(p, table, canonical, index=idx, index_bits=index_bits, num=1, den=1)
            d_wc = engine.window_counts(p, table, canonical, index=idx, index_bits=index_bits)
            try:
                mn = engine.record_quantile(p, d_wc, 0, 1)
            finally:
                d_wc.free()
        finally:
            idx.free()
        np.testing.assert_array_equal(st2, st)
        assert np.all(mn <= med) and np.all(med <= mx)
        plain = engine.emit_screen(p, st, None)
        assert plain == engine.emit_screen(p, st, None, median=None)
        return st, med, mn, mx, engine.emit_screen(p, st, None, median=med), plain
    finally:
        p.free()
        engine.free_result(table)


@pytest.mark.parametrize("canonical", [False, True])
def test_engine_screen_median_fasta(dev, canonical):
    k = 21
    reads = sc.records_of([150] * 40 + [0, 20, 21, 22, 0, C + 300, 150, 2 * C + 5], seed=5, prefix="read")
    reads[3] = (reads[3][0], sc.with_n(reads[3][1], [(40, 44), (100, 101)]))
    genome = [("chr1", "".join(s for _, s in reads[::2])), ("chr2", "".join(s for _, s in reads[:12])),
              ("chr3", reads[45][1][:C] + reads[47][1][200:])]
    table = sc.table_of(genome, k, canonical)
    want = sc.stats(reads, k, table, canonical)
    wmed = mc.medians(reads, k, table, canonical)
    assert 0 < want[:, 1].sum() < want[:, 0].sum() and {0, 1, 2} <= set(wmed)
    for bits in (None, 3):
        st, med, mn, mx, text, plain = _engine_median(dev, sc.fasta(reads), sc.fasta(genome), k, canonical,
                                                      index_bits=bits)
        np.testing.assert_array_equal(st, want)
        assert med.tolist() == wmed
        assert mn.tolist() == mc.medians(reads, k, table, canonical, 0, 1)
        assert mx.tolist() == mc.medians(reads, k, table, canonical, 1, 1)
        assert text == mc.lines(reads, want, wmed) and plain == sc.lines(reads, want)
        assert mc.property_holds(st, med)
    # only the solid k-mers of the table
    solid = sc.table_of(genome, k, canonical, min_count=2)
    st, med, _, _, text, _ = _engine_median(dev, sc.fasta(reads), sc.fasta(genome), k, canonical, min_count=2)
    assert med.tolist() == mc.medians(reads, k, solid, canonical) and mc.property_holds(st, med)
    assert text == mc.lines(reads, sc.stats(reads, k, solid, canonical), med)


@pytest.mark.parametrize("canonical, min_qual", [(False, 0), (True, 20)])
def test_engine_screen_median_fastq(dev, canonical, min_qual):
    import fastq_cases as fq
    from fastq_qual_cases import mask_fastq

    k = 11
    text = fq.mixed_reads(seed=3 + min_qual, n_records=120)
    fasta_text, n_masked = mask_fastq(text, min_qual, 33)
    assert (n_masked > 0) == (min_qual > 0)
    reads = sc.fasta_records(fasta_text)
    genome = [("g", "".join(s for _, s in sc.fasta_records(fq.fastq_to_fasta(text))[::3]))]
    table = sc.table_of(genome, k, canonical)
    want = sc.stats(reads, k, table, canonical)
    wmed = mc.medians(reads, k, table, canonical)
    assert 0 < sum(1 for m in wmed if m > 0) < len(reads)
    st, med, _, _, out, _ = _engine_median(dev, text, sc.fasta(genome), k, canonical, "fastq", min_qual)
    np.testing.assert_array_equal(st, want)
    assert med.tolist() == wmed and out == mc.lines(reads, want, wmed) and mc.property_holds(st, med)


def test_engine_record_quantile_refuses(dev):
    from kman_amd import engine

    p = engine.parse(dev, b">a\nACGTACGTAC\n")
    try:
        table = engine.join_groups(p, 4, False, "count")
        d_wc = engine.window_counts(p, table)
        try:
            for num, den in ((1, 0), (2, 1), (1, 65536), (-1, 2), (0.5, 1), (True, 2)):
                with pytest.raises(AssertionError):
                    engine.record_quantile(p, d_wc, num, den)
            assert engine.record_quantile(p, d_wc).tolist() == mc.medians([("a", "ACGTACGTAC")], 4,
                                                                          sc.table_of([("a", "ACGTACGTAC")], 4))
        finally:
            d_wc.free()
            engine.free_result(table)
    finally:
        p.free()


# ------------------------------------------------------------------------ CLI


def _cli(*argv):
    from kman_amd.scripts.kmer import main

    r = CliRunner().invoke(main, [str(a) for a in argv], catch_exceptions=False)
    assert r.exit_code == 0, r.output


def test_cli_median_end_to_end(tmp_path):
    k = 21
    reads = sc.records_of([150] * 40 + [10, 0, 21, C + 77], seed=21, prefix="read")
    reads += reads[5:9] + [("dup%d" % i, reads[2][1]) for i in range(3)]  # (repeated reads: medians above 1)
    # (an odd index, so not in the genome below: fewer than half of its windows are found, median 0 with hits)
    reads.append(("half", reads[0][1][:60] + sc.rand_seq(np.random.default_rng(22), 90)))
    assert len(reads) % 2 == 0
    genome = [("chr1", "".join(s for _, s in reads[::2])), ("chr2", "".join(s for _, s in reads[:10]))]
    (tmp_path / "reads.fa").write_bytes(sc.fasta(reads))
    (tmp_path / "genome.fa").write_bytes(sc.fasta(genome))
    with gzip.open(tmp_path / "genome.fa.gz", "wb") as fh:
        fh.write(sc.fasta(genome))
    out = tmp_path / "out.tsv"
    for canonical in (False, True):
        flags = ["--canonical"] if canonical else []
        table = sc.table_of(genome, k, canonical)
        want = sc.stats(reads, k, table, canonical)
        med = mc.medians(reads, k, table, canonical)
        assert mc.property_holds(want, med) and len({m for m in med}) >= 3
        _cli("screen", tmp_path / "reads.fa", tmp_path / "genome.fa.gz", out, k, "--median", *flags)
        assert out.read_bytes() == mc.lines(reads, want, med)
        # without the new options: today's bytes
        _cli("screen", tmp_path / "reads.fa", tmp_path / "genome.fa", out, k, *flags)
        assert out.read_bytes() == sc.lines(reads, want)
        solid = sc.table_of(genome, k, canonical, min_count=2)
        _cli("screen", tmp_path / "reads.fa", tmp_path / "genome.fa", out, k, "-L", 2, "--median", *flags)
        assert out.read_bytes() == mc.lines(reads, sc.stats(reads, k, solid, canonical),
                                            mc.medians(reads, k, solid, canonical))
        for argv, ka in ((["--min-median", 2], dict(min_median=2)), (["--max-median", 1], dict(max_median=1)),
                         (["--min-median", 1, "--max-median", 2], dict(min_median=1, max_median=2)),
                         (["--min-median", 1, "-v"], dict(min_median=1, invert=True)),
                         (["--max-median", 0, "--min-hits", 1], dict(max_median=0, min_hits=1)),
                         (["--median", "--min-frac", 0.5, "--min-median", 0], dict(min_frac=0.5, min_median=0))):
            kept = mc.keep(want, med, **ka)
            assert 0 < sum(kept) < len(reads), argv
            _cli("screen", tmp_path / "reads.fa", tmp_path / "genome.fa", out, k, *argv, *flags)
            assert out.read_bytes() == mc.lines(reads, want, med, kept), argv
    # self-screen: every record with a window has a median >= 1
    table = sc.table_of(reads, k, True)
    want, med = sc.stats(reads, k, table, True), mc.medians(reads, k, table, True)
    assert all((m >= 1) == (w > 0) for m, (w, _, _) in zip(med, want.tolist())) and max(med) >= 2
    _cli("screen", tmp_path / "reads.fa", tmp_path / "reads.fa", out, k, "--canonical", "--median")
    assert out.read_bytes() == mc.lines(reads, want, med)


def test_cli_median_fastq(tmp_path):
    import fastq_cases as fq
    from fastq_qual_cases import mask_fastq

    text = fq.mixed_reads(seed=8, n_records=80)
    (tmp_path / "reads.fq").write_bytes(text)
    with gzip.open(tmp_path / "reads.fq.gz", "wb") as fh:
        fh.write(text)
    k = 9
    fq_reads = sc.fasta_records(fq.fastq_to_fasta(text))
    genome = [("g", "".join(s for _, s in fq_reads[::2]))]
    with gzip.open(tmp_path / "g.fa.gz", "wb") as fh:
        fh.write(sc.fasta(genome))
    table = sc.table_of(genome, k)
    out = tmp_path / "out.tsv"
    for q, name in ((0, "reads.fq"), (20, "reads.fq.gz")):
        masked = sc.fasta_records(mask_fastq(text, q, 33)[0])
        want, med = sc.stats(masked, k, table), mc.medians(masked, k, table)
        assert mc.property_holds(want, med) and 0 < sum(1 for m in med if m) < len(med)
        _cli("screen", tmp_path / name, tmp_path / "g.fa.gz", out, k, "--median", *(["-q", q] if q else []))
        assert out.read_bytes() == mc.lines(masked, want, med), q
