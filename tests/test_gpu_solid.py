"""Per-read longest solid stretch on the GPU: kman_record_runs on hand-built
words, engine.screen_solid through the real kman_window_counts and `kmer
screen --solid / --min-solid-len / --bed`, all for equality with the
plain-Python statement (tests/solid_cases.py)."""

from __future__ import annotations

import gzip
from ctypes import byref, c_uint64, c_void_p

import numpy as np
import pytest
from click.testing import CliRunner

import median_cases as mc
import screen_cases as sc
import solid_cases as so

pytestmark = pytest.mark.gpu

from kman_amd import _native as N  # noqa: E402

T = N.KMAN_RUNS_TILE
CAP = N.KMAN_RUNS_REC_CAP
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


def _plan(n_bases, n_records):
    out = c_uint64(0)
    assert N.lib().kman_record_runs_plan(n_bases, n_records, byref(out)) == N.KMAN_OK
    return out.value


def _runs(dev, words, rec_seq, n_bases, min_count, work_bytes=None, n_records=None, null=None):
    """One kman_record_runs call: (return code, the (R, 2) rows (start, len),
    the raw planes with the sentinel words after them).  The words and the
    sentinel words after them must come back unchanged."""
    words = np.ascontiguousarray(words, dtype=np.uint32)
    rec_seq = np.ascontiguousarray(rec_seq, dtype=np.uint64)
    R = len(rec_seq)
    plan = _plan(n_bases, R)
    if work_bytes is None:
        work_bytes = plan
    padded = np.concatenate([words, np.full(PAD, SENT32, np.uint32)])
    bufs = [_up(dev, padded), _up(dev, rec_seq), dev.alloc(max(16, plan)),
            _up(dev, np.full(2 * R + PAD, SENT64, np.uint64))]
    try:
        ptrs = [b.ptr for b in bufs]
        if null is not None:
            ptrs[null] = None
        rc = N.lib().kman_record_runs(dev.ctx, c_void_p(ptrs[0]), n_bases, c_void_p(ptrs[1]),
                                      R if n_records is None else n_records, min_count, c_void_p(ptrs[2]), work_bytes,
                                      c_void_p(ptrs[3]))
        raw = dev.download(bufs[3], 2 * R + PAD, np.uint64)
        np.testing.assert_array_equal(dev.download(bufs[0], len(padded), np.uint32), padded)  # d_wc is not modified
        return rc, np.ascontiguousarray(raw[:2 * R].reshape(2, R).T), raw
    finally:
        for b in bufs:
            b.free()


def _check(dev, words, rec_seq, n_bases, min_count=1):
    """The call against the statement; the rows."""
    words = np.ascontiguousarray(words, dtype=np.uint32)
    assert len(words) >= n_bases
    rc, got, raw = _runs(dev, words, rec_seq, n_bases, min_count)
    assert rc == N.KMAN_OK, N.lib().kman_last_error(dev.ctx)
    assert np.all(raw[2 * len(rec_seq):] == SENT64)  # words past the planes untouched
    want = so.record_runs(words[:n_bases].tolist(), rec_seq, n_bases, min_count)
    assert [tuple(x) for x in got.tolist()] == want
    return want


def _words(n, runs, val=5, fill=NONE):
    """n words of `fill` with [a, b) set to `val` for every run."""
    w = np.full(n, fill, np.uint32)
    for a, b in runs:
        w[a:b] = val
    return w


# ------------------------------------------------------------ runs and tiles


@pytest.mark.parametrize("last", [T - 1, T, T + 1])
def test_run_ending_around_a_tile_edge(dev, last):
    n = 2 * T + 10
    want = _check(dev, _words(n, [(T - 50, last + 1), (10, 20)]), [0], n)
    assert want == [(T - 50, last + 1 - (T - 50))]
    # the same run as the whole of a record that starts in mid-tile, its neighbours solid
    w = _words(n, [(0, n)])
    assert _check(dev, w, [0, T - 50, last + 1], n) == [(0, T - 50), (0, last + 51 - T), (0, n - last - 1)]


def test_run_across_a_tile_edge_and_over_three_tiles(dev):
    n = 5 * T
    assert _check(dev, _words(n, [(T - 1, T + 2)]), [0], n) == [(T - 1, 3)]
    # three tiles inside a longer record, shorter runs before and after it
    w = _words(n, [(5, 300), (T - 100, 3 * T + 50), (3 * T + 60, 4 * T + 7), (4 * T + 100, 5 * T)])
    assert _check(dev, w, [0], n) == [(T - 100, 2 * T + 150)]
    # the run starts exactly on a tile's first base and ends on a tile's last
    assert _check(dev, _words(n, [(T, 3 * T), (3 * T + 1, 4 * T)]), [0], n) == [(T, 2 * T)]
    # a low word, not a NONE, ends it
    w = _words(n, [(0, n)], val=7)
    w[3 * T + 9] = 6
    assert _check(dev, w, [0], n, 7) == [(0, 3 * T + 9)]
    assert _check(dev, w, [0], n, 6) == [(0, n)]


def test_run_covering_a_whole_record(dev):
    L = 3 * T + 5
    n = 7 + L + 20
    w = _words(n, [(0, n)])  # no NONE anywhere: only the record table cuts
    assert _check(dev, w, [0, 7, 7 + L], n) == [(0, 7), (0, L), (0, 20)]
    assert _check(dev, w, [7, 7 + L], n) == [(0, L), (0, 20)]
    # the same record with one weak base: the longer side, and the tie when it sits in the middle
    w[7 + 2 * T] = 0
    assert _check(dev, w, [0, 7, 7 + L], n) == [(0, 7), (0, 2 * T), (0, 20)]
    w = _words(n, [(0, n)])
    w[7 + L // 2] = NONE
    assert L % 2 == 1 and _check(dev, w, [0, 7, 7 + L], n) == [(0, 7), (0, L // 2), (0, 20)]


def test_thread_and_wave_edges(dev):
    n = 3 * T
    edges = [16, 32, 1024, 2048, T + 16, T + 1024]
    for e in edges:
        for runs in ([(e - 7, e)], [(e, e + 7)], [(e - 1, e + 1)], [(e - 16, e + 16)], [(e - 7, e), (e + 1, e + 8)],
                     [(e - 7, e), (e + 1, e + 9)]):
            want = _check(dev, _words(n, runs), [0], n)
            best = max(runs, key=lambda r: (r[1] - r[0], -r[0]))
            assert want == [(best[0], best[1] - best[0])], (e, runs)
    # every thread's 16 words are one run of their own: 15 solid, one weak, at each position of the weak one
    for at in (0, 7, 15):
        w = _words(n, [(0, n)])
        w[at::16] = 1
        assert _check(dev, w, [0], n, 2) == [(0 if at == 15 else at + 1, 15)]


def test_ties(dev):
    n = 3 * T
    # two equal runs in one thread's 16 words, a third one later
    assert _check(dev, _words(n, [(2, 5), (8, 11), (T + 40, T + 43)]), [0], n) == [(2, 3)]
    assert _check(dev, _words(n, [(T + 34, T + 37), (T + 40, T + 43)]), [0, T + 32], n) == [(0, 0), (2, 3)]
    # equal runs in different tiles of one record: the leftmost
    assert _check(dev, _words(n, [(100, 200), (T + 300, T + 400), (2 * T + 1, 2 * T + 101)]), [0], n) == [(100, 100)]
    assert _check(dev, _words(n, [(T - 50, T + 50), (2 * T - 50, 2 * T + 50)]), [0], n) == [(T - 50, 100)]
    # a longer run later wins
    assert _check(dev, _words(n, [(100, 200), (2 * T + 5, 2 * T + 106)]), [0], n) == [(2 * T + 5, 101)]
    assert _check(dev, _words(n, [(100, 200), (300, 401)]), [0], n) == [(300, 101)]
    # the same with the record starting in an earlier tile than its runs, and two such records
    rs = [0, 50, T + 100]
    w = _words(n, [(60, 90), (T - 10, T + 20), (T + 200, T + 230), (2 * T + 200, 2 * T + 230), (2 * T + 300, 2 * T + 331)])
    assert _check(dev, w, rs, n) == [(0, 0), (10, 30), (2 * T + 300 - (T + 100), 31)]


def test_record_cuts(dev):
    n = 3 * T + 100
    w = _words(n, [(0, n)])  # solid on both sides of every boundary, no NONE between
    assert _check(dev, w, [0, 1000], n) == [(0, 1000), (0, n - 1000)]
    assert _check(dev, w, [0, T], n) == [(0, T), (0, n - T)]
    assert _check(dev, w, [0, T - 1, T, T + 1], n) == [(0, T - 1), (0, 1), (0, 1), (0, n - T - 1)]
    assert _check(dev, w, [0, T - 1, T + 1, 2 * T, 3 * T], n) == [(0, T - 1), (0, 2), (0, T - 1), (0, T), (0, 100)]
    for s in (T - 1, T, T + 1):
        assert _check(dev, w, [s], n) == [(0, n - s)]
        assert _check(dev, w, [5, s, s + 40], n) == [(0, s - 5), (0, 40), (0, n - s - 40)]
    # a weak base right before, on, and right after a boundary
    for weak, want in ((T - 1, [(0, T - 1), (0, n - T)]), (T, [(0, T), (1, n - T - 1)]),
                       (T + 1, [(0, T), (2, n - T - 2)])):
        v = w.copy()
        v[weak] = NONE
        assert _check(dev, v, [0, T], n) == want


def test_thresholds(dev):
    n = T + 300
    rng = np.random.default_rng(1)
    for mc_ in (1, 2, 3, 1000, 1 << 31, SAT):
        w = np.where(rng.random(n) < 0.7, np.uint32(mc_), np.uint32(mc_ - 1)).astype(np.uint32)
        want = _check(dev, w, [0, 150, 300, T - 5], n, mc_)
        assert max(x[1] for x in want) > 1
        if mc_ > 1:
            assert _check(dev, w, [0], n, mc_ - 1) == [(0, n)]  # one lower: every word is solid
    w = np.tile(np.asarray([SAT, SAT, SAT - 1, NONE, SAT, SAT, SAT, NONE, 0], np.uint32), 40)
    assert _check(dev, w, [0], len(w), SAT) == [(4, 3)]
    assert _check(dev, w, [0], len(w), SAT - 1) == [(0, 3)]
    assert _check(dev, w, [0], len(w), 1) == [(0, 3)]   # min_count 1: NONE and 0 are the only weak words


def test_uniform_words(dev):
    n = 2 * T + 77
    rs = [0, 150, 150, 300, T - 1, T + 1, 2 * T]
    assert _check(dev, np.full(n, NONE, np.uint32), rs, n) == [(0, 0)] * len(rs)
    assert _check(dev, np.zeros(n, np.uint32), rs, n) == [(0, 0)] * len(rs)
    ends = rs[1:] + [n]
    assert _check(dev, np.full(n, 9, np.uint32), rs, n, 9) == [(0, e - s) for s, e in zip(rs, ends)]
    for first in (0, 1):  # every other word solid: the first solid base of every record
        w = np.full(n, NONE, np.uint32)
        w[first::2] = 3
        want = _check(dev, w, rs, n)
        assert want == [((s + first) % 2, 1) if e > s else (0, 0) for s, e in zip(rs, ends)]


def test_record_table_edges(dev):
    n = T + 200
    rng = np.random.default_rng(2)
    w = np.where(rng.random(n) < 0.9, np.uint32(4), NONE).astype(np.uint32)
    # empty records and repeated entries (the last owns the bases), at the start, in the middle, at the end
    _check(dev, w, [0, 0, 0, 100, 100, 250, T, T, T + 10, T + 200 - 1, T + 200 - 1], n)
    # a record that starts at n_bases, and entries above it (clamped)
    want = _check(dev, w, [0, 500, n, n, n + 5, 1 << 40], n)
    assert want[2:] == [(0, 0)] * 4 and want[1][1] > 0
    # bases before the first entry belong to nobody
    w2 = _words(n, [(0, 50), (60, 70), (T - 3, T + 9)])
    assert _check(dev, w2, [40, 65, T], n) == [(0, 10), (0, 5), (0, 9)]
    assert _check(dev, w2, [T + 100], n) == [(0, 0)]
    assert _check(dev, w2, [T + 2, T + 2], n) == [(0, 0), (0, 7)]
    # only empty records; every record beyond the bases
    assert _check(dev, w, [n] * 5, n) == [(0, 0)] * 5
    assert _check(dev, w, [n + 1, n + 2], n) == [(0, 0)] * 2


@pytest.mark.parametrize("name", ["cap", "cap_plus_1", "many", "many_carry"])
def test_more_records_in_a_tile_than_the_lds_slice(dev, name):
    if name in ("cap", "cap_plus_1"):
        R = CAP + (name == "cap_plus_1")
        rec_seq = np.arange(R, dtype=np.uint64)  # one-base records; the last one takes the rest
        n = R + 40
    else:
        lead = [150, 150] if name == "many" else [T - 10, 150]
        lens = lead + [1, 0, 2] * (CAP + 3) + [150, 33]
        rec_seq = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.uint64)
        n = int(sum(lens))
        per_tile = np.bincount((rec_seq // T).astype(np.int64))
        assert per_tile[0 if name == "many" else 1] > CAP
    rng = np.random.default_rng(len(name))
    w = np.where(rng.random(n) < 0.8, np.uint32(2), np.uint32(1)).astype(np.uint32)
    want = _check(dev, w, rec_seq, n, 2)
    assert {(0, 0), (0, 1)} <= set(want)
    _check(dev, np.full(n, 2, np.uint32), rec_seq, n, 2)


def test_tiny_and_empty_inputs(dev):
    assert _check(dev, [7], [0], 1) == [(0, 1)]
    assert _check(dev, [7], [0], 1, 8) == [(0, 0)]
    assert _check(dev, [NONE], [0], 1) == [(0, 0)]
    # n_bases == 0: both planes are zeroed, the word and work pointers may be NULL
    assert _check(dev, [], [0, 0, 5], 0) == [(0, 0)] * 3
    for null in (0, 2):
        rc, got, raw = _runs(dev, [], [0, 0, 5], 0, 1, null=null)
        assert rc == N.KMAN_OK and not got.any() and np.all(raw[6:] == SENT64)
    # n_records == 0: nothing is done
    rc, got, raw = _runs(dev, _words(100, [(0, 100)]), [0, 50], 100, 1, n_records=0)
    assert rc == N.KMAN_OK and np.all(raw == SENT64)


LAYOUTS = {
    # name: (bases before the first record, record lengths)
    "reads150": (0, [150] * 60 + [37]),
    "mixed": (3, [0, 1, 2, T - 1, T, T + 1, 0, 5, 150, 3]),
    "tile_edges": (0, [T, T - 101, 100, 1, 300, T - 300, T, 150, 37]),
    "long_between_short": (7, [10, 3 * T + 500, 20, 0, 2 * T, 5]),
    "end_at_tile": (0, [T, T - 5, 5, T, 0]),
}


@pytest.mark.parametrize("name", sorted(LAYOUTS))
def test_random_words_on_record_layouts(dev, name):
    lead, lengths = LAYOUTS[name]
    rec_seq = (lead + np.concatenate([[0], np.cumsum(lengths)[:-1]])).astype(np.uint64)
    n = lead + int(sum(lengths))
    rng = np.random.default_rng(len(name))
    for p_weak in (0.5, 0.05, 0.002):  # runs of a few bases, of a thread's words, of tiles
        w = rng.choice(np.asarray([1, 2, 3, 7, SAT], np.uint32), n)
        weak = rng.random(n) < p_weak
        w[weak] = rng.choice(np.asarray([0, NONE], np.uint32), int(weak.sum()))
        for mc_ in (1, 3):
            _check(dev, w, rec_seq, n, mc_)
    w = np.full(n, 2, np.uint32)
    a = _runs(dev, w, rec_seq, n, 2)[2]
    b = _runs(dev, w, rec_seq, n, 2)[2]
    assert a.tobytes() == b.tobytes()  # two calls: identical bytes


def test_refusals_write_nothing(dev):
    n = 2 * T + 9
    w = _words(n, [(3, T + 70), (T + 90, n)])
    rs = [0, 100, T + 5]
    want = so.record_runs(w.tolist(), rs, n, 1)
    plan = _plan(n, len(rs))
    assert plan >= 16 and plan % 16 == 0
    for kw, code in ((dict(min_count=0), N.KMAN_EINVAL), (dict(min_count=0xFFFFFFFF), N.KMAN_EINVAL),
                     (dict(work_bytes=plan - 1), N.KMAN_ECAP), (dict(work_bytes=0), N.KMAN_ECAP),
                     (dict(null=0), N.KMAN_EINVAL), (dict(null=1), N.KMAN_EINVAL), (dict(null=2), N.KMAN_EINVAL),
                     (dict(null=3), N.KMAN_EINVAL)):
        args = dict(min_count=1)
        args.update(kw)
        rc, _, raw = _runs(dev, w, rs, n, **args)
        assert rc == code, kw
        assert np.all(raw == SENT64), kw  # the outputs untouched
    rc, got, _ = _runs(dev, w, rs, n, 1)  # the context is still usable
    assert rc == N.KMAN_OK and [tuple(x) for x in got.tolist()] == want
    rc, got, _ = _runs(dev, w, rs, n, 1, work_bytes=plan + 4096)
    assert rc == N.KMAN_OK and [tuple(x) for x in got.tolist()] == want


# ------------------------------------------------------------------ engine API


def _table(dev, table_text, k, canonical):
    from kman_amd import engine

    p = engine.parse(dev, table_text)
    try:
        table = engine.join_groups(p, k, False, "count", canonical=canonical)
    finally:
        p.free()
    return table if table is not None else engine.empty_count(dev, k)


def _engine_solid(dev, reads_text, table_text, k, min_count, canonical=False, fmt="auto", min_qual=0):
    """engine.screen_solid with and without the median: (stats, median, runs, the text, the BED)."""
    from kman_amd import engine

    table = _table(dev, table_text, k, canonical)
    p = engine.parse(dev, reads_text, fmt, min_qual)
    try:
        st, none, runs = engine.screen_solid(p, table, canonical, min_count)
        assert none is None and st.shape == (p.n_records, 3)
        assert runs.shape == (p.n_records, 2) and runs.dtype == np.uint64
        st2, med, runs2 = engine.screen_solid(p, table, canonical, min_count, median=True)
        want_st, want_med = engine.screen_median(p, table, canonical)
        np.testing.assert_array_equal(st, want_st)
        np.testing.assert_array_equal(st2, want_st)
        np.testing.assert_array_equal(med, want_med)
        np.testing.assert_array_equal(runs2, runs)
        idx = engine.table_index(dev, table, 3)
        try:
            st3, _, runs3 = engine.screen_solid(p, table, canonical, min_count, index=idx, index_bits=3)
        finally:
            idx.free()
        np.testing.assert_array_equal(st3, st)
        np.testing.assert_array_equal(runs3, runs)
        span = engine.solid_spans(runs, k)
        text = engine.emit_screen(p, st, None, span=span)
        text_med = engine.emit_screen(p, st, None, median=med, span=span)
        return st, med, runs, text, text_med, engine.emit_bed(p, span, None)
    finally:
        p.free()
        engine.free_result(table)


def _multiline(records, width=60) -> bytes:
    out = []
    for name, seq in records:
        out.append(">%s\n" % name)
        out += [seq[i:i + width] + "\n" for i in range(0, len(seq), width)]
    return "".join(out).encode()


@pytest.mark.parametrize("canonical", [False, True])
@pytest.mark.parametrize("k", [2, 3, 21, 31, 32])
def test_engine_screen_solid_fasta(dev, k, canonical):
    rng = np.random.default_rng(k)
    reads = sc.records_of([150] * 12 + [0, k - 1, k, k + 1, 400, T + 300], seed=40 + k, prefix="read")
    reads[2] = (reads[2][0], sc.with_n(reads[2][1], [(70, 71)]))            # one N in mid-read
    reads[3] = (reads[3][0], sc.with_n(reads[3][1], [(0, 1), (100, 104)]))
    bad = list(reads[4][1])                                                 # one wrong base: k weak windows
    bad[90] = "ACGT"[("ACGT".index(bad[90]) + 1) % 4]
    reads.append(("err", "".join(bad)))
    reads.append(("novel", sc.rand_seq(rng, 120)))
    genome = [("g%d" % i, "".join(s for _, s in reads[:18])) for i in range(3)] + [("once", reads[5][1])]
    table = sc.table_of(genome, k, canonical)
    for min_count, text_of in ((3, _multiline), (4, sc.fasta)):
        want = so.runs_of(reads, k, table, min_count, canonical)
        span = so.spans(want, k)
        if k >= 21 and min_count == 3:
            assert want[-2] == (0, 90 - k + 1) and want[-1] == (0, 0) and want[2] == (71, 80 - k)
            assert span[0] == (0, 150) and span[-2] == (0, 90) and span[2] == (71, 150)
        if k >= 21 and min_count == 4:  # only the read that the table holds once more
            assert [r for r, (_, n) in enumerate(want) if n] == [5]
        st, med, runs, text, text_med, bed = _engine_solid(dev, text_of(reads), sc.fasta(genome), k, min_count,
                                                           canonical)
        assert [tuple(x) for x in runs.tolist()] == want
        stats = sc.stats(reads, k, table, canonical)
        np.testing.assert_array_equal(st, stats)
        assert med.tolist() == mc.medians(reads, k, table, canonical)
        assert text == so.lines(reads, stats, span) and text_med == so.lines(reads, stats, span, med)
        assert bed == so.bed(reads, span)
        for (name, seq), (a, b) in zip(reads, span):  # every window of a span is solid, the ones beside it are not
            if b > a:
                ws = mc.window_words([(name, seq)], k, table, canonical)
                assert all(so.solid(x, min_count) for x in ws[a:b - k + 1]) and b <= len(seq)
                assert a == 0 or not so.solid(ws[a - 1], min_count)
                assert b - k + 1 >= len(ws) or not so.solid(ws[b - k + 1], min_count)


@pytest.mark.parametrize("canonical, min_qual", [(False, 0), (True, 20)])
def test_engine_screen_solid_fastq(dev, canonical, min_qual):
    import fastq_cases as fq
    from fastq_qual_cases import mask_fastq

    k = 11
    text = fq.mixed_reads(seed=5 + min_qual, n_records=100)
    fasta_text, n_masked = mask_fastq(text, min_qual, 33)
    assert (n_masked > 0) == (min_qual > 0)
    reads = sc.fasta_records(fasta_text)       # (masked bases are N: they end a stretch)
    plain = sc.fasta_records(fq.fastq_to_fasta(text))
    genome = [("g", "".join(s for _, s in plain)), ("h", "".join(s for _, s in plain[::2]))]
    table = sc.table_of(genome, k, canonical)
    want = so.runs_of(reads, k, table, 2, canonical)
    span = so.spans(want, k)
    if min_qual:
        cut = [r for r, ((_, a), (_, b)) in enumerate(zip(reads, plain)) if a != b and len(a) >= k]
        unmasked = so.runs_of(plain, k, table, 2, canonical)
        assert any("N" in reads[r][1][1:-1] and want[r][1] < unmasked[r][1] for r in cut)  # a base masked in mid-read
    st, med, runs, out, _, bed = _engine_solid(dev, text, sc.fasta(genome), k, 2, canonical, "fastq", min_qual)
    assert [tuple(x) for x in runs.tolist()] == want
    stats = sc.stats(reads, k, table, canonical)
    np.testing.assert_array_equal(st, stats)
    assert out == so.lines(reads, stats, span) and bed == so.bed(reads, span)
    assert 0 < sum(1 for _, n in want if n) and len({n for _, n in want}) > 3


def test_engine_record_runs_refuses(dev):
    from kman_amd import engine

    p = engine.parse(dev, b">a\nACGTACGTAC\n>b\n>c\nACGTTT\n")
    try:
        table = engine.join_groups(p, 4, False, "count")
        d_wc = engine.window_counts(p, table)
        try:
            for bad in (0, -1, 0xFFFFFFFF, 1 << 40, 1.5, True, None):
                with pytest.raises(AssertionError):
                    engine.record_runs(p, d_wc, bad)
                with pytest.raises(AssertionError):
                    engine.screen_solid(p, table, False, bad)
            recs = [("a", "ACGTACGTAC"), ("b", ""), ("c", "ACGTTT")]
            t = sc.table_of(recs, 4)
            for mc_ in (1, 2, 3, SAT):
                assert [tuple(x) for x in engine.record_runs(p, d_wc, mc_).tolist()] == so.runs_of(recs, 4, t, mc_)
            # runs first, the quantile after them on the same words
            assert engine.record_quantile(p, d_wc).tolist() == mc.medians(recs, 4, t)
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


def test_cli_solid_end_to_end(tmp_path):
    k = 21
    rng = np.random.default_rng(31)
    reads = sc.records_of([150] * 30 + [10, 0, 21, T + 77], seed=33, prefix="read")
    for i in (3, 8, 13):  # a wrong base at 40, 75 and 140
        s = list(reads[i][1])
        at = (40, 75, 140)[(3, 8, 13).index(i)]
        s[at] = "ACGT"[("ACGT".index(s[at]) + 2) % 4]
        reads.append(("err%d" % i, "".join(s)))
    reads.append(("novel", sc.rand_seq(rng, 150)))
    reads.append(("withN", sc.with_n(reads[5][1], [(60, 62)])))
    genome = [("chr%d" % i, "".join(s for _, s in reads[:34])) for i in range(3)]
    (tmp_path / "reads.fa").write_bytes(_multiline(reads, 70))
    with gzip.open(tmp_path / "reads.fa.gz", "wb") as fh:
        fh.write(sc.fasta(reads))
    (tmp_path / "genome.fa").write_bytes(sc.fasta(genome))
    out, bed = tmp_path / "out.tsv", tmp_path / "out.bed"
    for canonical in (False, True):
        flags = ["--canonical"] if canonical else []
        table = sc.table_of(genome, k, canonical)
        stats = sc.stats(reads, k, table, canonical)
        med = mc.medians(reads, k, table, canonical)
        span = so.spans(so.runs_of(reads, k, table, 3, canonical), k)
        assert span[34:] == [(41, 150), (0, 75), (0, 140), (0, 0), (62, 150)] and span[0] == (0, 150)
        _cli("screen", tmp_path / "reads.fa", tmp_path / "genome.fa", out, k, "--solid", 3, *flags)
        assert out.read_bytes() == so.lines(reads, stats, span) and not bed.exists()
        # gzipped one-line input: the same coordinates (line breaks do not count)
        _cli("screen", tmp_path / "reads.fa.gz", tmp_path / "genome.fa", out, k, "--solid", 3, "--bed", bed, *flags)
        assert out.read_bytes() == so.lines(reads, stats, span) and bed.read_bytes() == so.bed(reads, span)
        assert reads[34][1][41:150] == reads[3][1][41:]  # what the BED line of err3 cuts out: the read after its error
        # the columns after the median
        _cli("screen", tmp_path / "reads.fa", tmp_path / "genome.fa", out, k, "--solid", 3, "--median", *flags)
        assert out.read_bytes() == so.lines(reads, stats, span, med)
        # without --solid: the bytes of the same command before the option existed
        _cli("screen", tmp_path / "reads.fa", tmp_path / "genome.fa", out, k, *flags)
        assert out.read_bytes() == sc.lines(reads, stats)
        _cli("screen", tmp_path / "reads.fa", tmp_path / "genome.fa", out, k, "--median", *flags)
        assert out.read_bytes() == mc.lines(reads, stats, med)
        for argv, ka in ((["--min-solid-len", 100], dict(min_solid_len=100)),
                         (["--min-solid-len", 100, "-v"], dict(min_solid_len=100, invert=True)),
                         (["--min-solid-len", 141], dict(min_solid_len=141)),
                         (["--min-solid-len", 0, "--min-hits", 1], dict(min_solid_len=0, min_hits=1)),
                         (["--min-solid-len", 1, "--max-median", 3, "--min-frac", 0.5],
                          dict(min_solid_len=1, med=med, max_median=3, min_frac=0.5))):
            kept = so.keep(stats, span, **ka)
            assert 0 < sum(kept) < len(reads), argv
            with_med = med if "--max-median" in argv else None
            _cli("screen", tmp_path / "reads.fa", tmp_path / "genome.fa", out, k, "--solid", 3, "--bed", bed, *argv,
                 *flags)
            assert out.read_bytes() == so.lines(reads, stats, span, with_med, kept), argv
            assert bed.read_bytes() == so.bed(reads, span, kept), argv
        # another threshold: the table's k-mers have a count of 3 (the genome holds every read three times), none reaches 7
        _cli("screen", tmp_path / "reads.fa", tmp_path / "genome.fa", out, k, "--solid", 7, "--bed", bed, *flags)
        none = so.spans(so.runs_of(reads, k, table, 7, canonical), k)
        assert out.read_bytes() == so.lines(reads, stats, none)
        assert bed.read_bytes() == so.bed(reads, none)
        bed.unlink()


def test_cli_solid_fastq_self_screen(tmp_path):
    """Self-screened error trimming: READS = TABLE_INPUT, --canonical, -q masks bases into N."""
    import fastq_cases as fq
    from fastq_qual_cases import mask_fastq

    text = fq.mixed_reads(seed=9, n_records=60)
    (tmp_path / "reads.fq").write_bytes(text + text)  # every read twice: its k-mers reach 2
    k = 9
    out, bed = tmp_path / "out.tsv", tmp_path / "out.bed"
    for q in (0, 20):
        masked = sc.fasta_records(mask_fastq(text + text, q, 33)[0])
        table = sc.table_of(masked, k, True)
        stats = sc.stats(masked, k, table, True)
        span = so.spans(so.runs_of(masked, k, table, 2, True), k)
        assert sum(1 for a, b in span if b > a) > 10
        _cli("screen", tmp_path / "reads.fq", tmp_path / "reads.fq", out, k, "--canonical", "--solid", 2, "--bed", bed,
             *(["-q", q] if q else []))
        assert out.read_bytes() == so.lines(masked, stats, span), q
        assert bed.read_bytes() == so.bed(masked, span), q
