"""Reads against a table on the GPU: kman_table_index against np.searchsorted,
kman_screen_records, engine.screen / emit_screen and `kmer screen` against the
plain-Python statement (tests/screen_cases.py), all for equality."""

from __future__ import annotations

import functools
import gzip
from ctypes import c_void_p

import numpy as np
import pytest
from click.testing import CliRunner

import screen_cases as sc

pytestmark = pytest.mark.gpu

from kman_amd import _native as N  # noqa: E402

T = N.KMAN_SCREEN_TILE
CAP = N.KMAN_SCREEN_REC_CAP
MAXB = N.KMAN_SCREEN_MAX_INDEX_BITS
PAD = 16  # sentinel words after an output
SENT = 0xA5A5A5A5A5A5A5A5


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


# ------------------------------------------------------------ kman_table_index


def _table_index(dev, keys, k, bits):
    keys = np.asarray(keys, dtype=np.uint64)
    n = (1 << bits) + 1 if 0 < bits <= MAXB else 2
    dk = _up(dev, keys)
    out = dev.alloc(8 * (n + PAD))
    dev.memset(out, 0xA5, 8 * (n + PAD))  # (every byte of SENT)
    try:
        rc = N.lib().kman_table_index(dev.ctx, c_void_p(dk.ptr), len(keys), k, bits, c_void_p(out.ptr))
        return rc, dev.download(out, n + PAD, np.uint64)
    finally:
        dk.free()
        out.free()


def _index_tables(k, bits):
    kb = 2 * k
    top, per = (1 << kb) - 1, 1 << (kb - bits)
    rng = np.random.default_rng(kb * 100 + bits)
    mid = (1 << bits) // 2
    yield "empty", []
    yield "one_row", [top // 3]
    yield "three_rows_with_both_extremes", sorted({0, top // 2, top})
    yield "one_bucket", [mid * per + i for i in range(min(5000, per))]
    yield "first_and_last_bucket", sorted({i for i in range(min(per, 40))} | {top - i for i in range(min(per, 40))})
    if kb <= 16:
        yield "random", sorted(set(rng.integers(0, top + 1, (top + 1) // 2).tolist()))
    else:
        hi = rng.integers(0, 1 << 32, 3000, dtype=np.uint64).astype(object)
        lo = rng.integers(0, 1 << 32, 3000, dtype=np.uint64).astype(object)
        yield "random", sorted({int((h << 32 | l) & top) for h, l in zip(hi, lo)} | {0, top})


@pytest.mark.parametrize("k, bits", [(2, 1), (2, 4), (3, 1), (3, 6), (16, 1), (16, 24), (21, 13), (32, 1), (32, 24)])
def test_table_index_against_searchsorted(dev, k, bits):
    shift = 2 * k - bits
    bounds = np.arange(1 << bits, dtype=np.uint64) << np.uint64(shift)
    one_bucket_rows = 0
    for name, rows in _index_tables(k, bits):
        if bits == MAXB and name in ("empty", "one_row", "three_rows_with_both_extremes"):
            continue  # (the small tables at the narrower widths; a 2^24-entry index is 128 MiB to compare)
        keys = np.asarray(rows, dtype=np.uint64)
        assert np.all(keys[1:] > keys[:-1]), name
        want = np.concatenate([np.searchsorted(keys, bounds, side="left"), [len(keys)]]).astype(np.uint64)
        rc, got = _table_index(dev, keys, k, bits)
        assert rc == N.KMAN_OK, name
        np.testing.assert_array_equal(got[:-PAD], want, err_msg=name)
        assert np.all(got[-PAD:] == SENT), name
        if name == "one_bucket":
            one_bucket_rows = int(np.diff(want.astype(np.int64)).max())
            assert one_bucket_rows == len(keys)
    if (k, bits) in ((32, 24), (32, 1), (21, 13)):
        assert one_bucket_rows == 5000  # (a bucket larger than any small fixed step count)


def test_table_index_refused(dev):
    keys = np.asarray([1, 5, 9], dtype=np.uint64)
    for k, bits in ((2, 0), (2, 5), (3, 0), (3, 7), (16, 25), (32, 25), (1, 1), (33, 8)):
        rc, got = _table_index(dev, keys, k, bits)
        assert rc == N.KMAN_EINVAL, (k, bits)
        assert np.all(got == SENT)  # nothing was written
    rc, got = _table_index(dev, keys, 16, 3)  # the context is still usable
    assert rc == N.KMAN_OK and got[:9].tolist() == [0, 3, 3, 3, 3, 3, 3, 3, 3]


# -------------------------------------------------------- kman_screen_records


def _screen(dev, records, k, table, canonical=False, cb=4, bits=None, twice=False):
    """kman_screen_records on the helper's device layout of `records`, the
    output pre-filled with a nonzero pattern; the (n_records, 3) result."""
    from kman_amd import engine

    codes, rec_seq, n_bases = sc.codes_of(records)
    keys, counts = sc.table_rows(table, cb)
    R = len(records)
    if bits is None:
        bits = engine.default_index_bits(len(keys), k)
    L = N.lib()
    bufs = [_up(dev, codes), _up(dev, rec_seq), _up(dev, keys), _up(dev, counts),
            dev.alloc(8 * ((1 << bits) + 1)), None]
    try:
        d_codes, d_rec, d_keys, d_counts, d_index, _ = bufs
        assert L.kman_table_index(dev.ctx, c_void_p(d_keys.ptr), len(keys), k, bits, c_void_p(d_index.ptr)) == N.KMAN_OK
        fill = np.full(3 * R + PAD, SENT, np.uint64)
        runs = []
        for _ in range(2 if twice else 1):
            d_out = bufs[5] = _up(dev, fill)
            rc = L.kman_screen_records(dev.ctx, c_void_p(d_codes.ptr), n_bases, k, N.KMAN_CANONICAL if canonical else 0,
                                       c_void_p(d_rec.ptr), R, c_void_p(d_keys.ptr), c_void_p(d_counts.ptr), cb,
                                       len(keys), c_void_p(d_index.ptr), bits, c_void_p(d_out.ptr))
            assert rc == N.KMAN_OK, N.lib().kman_last_error(dev.ctx)
            got = dev.download(d_out, 3 * R + PAD, np.uint64)
            d_out.free()
            bufs[5] = None
            assert np.all(got[3 * R:] == SENT)  # nothing past the three planes
            runs.append(got[:3 * R])
        if twice:
            assert runs[0].tobytes() == runs[1].tobytes()  # the same call twice: identical bytes
        np.testing.assert_array_equal(dev.download(d_rec, R, np.uint64), rec_seq)  # (inputs are not written)
        return np.ascontiguousarray(runs[0].reshape(3, R).T)
    finally:
        for b in bufs:
            if b is not None:
                b.free()


def _half_table(records, k, canonical, seed=9, count_add=0):
    """The k-mers of every second record that has any, and unrelated sequence."""
    own = [r for r in records if len(r[1]) >= k][::2]
    t = sc.table_of(own + sc.records_of([400, 300], seed, "x"), k, canonical)
    return {w: c + count_add for w, c in t.items()}


def _check(dev, records, k, table, canonical=False, cb=4, bits=None, twice=False):
    want = sc.stats(records, k, table, canonical)
    got = _screen(dev, records, k, table, canonical, cb, bits, twice)
    np.testing.assert_array_equal(got, want)
    return want


LAYOUTS = sorted(sc.layouts(5, T, CAP))


@pytest.mark.parametrize("k", [5, 21])
@pytest.mark.parametrize("name", LAYOUTS)
def test_record_layouts(dev, name, k):
    lengths = sc.layouts(k, T, CAP)[name]
    records = sc.records_of(lengths, seed=len(name) + k)
    _, rec_seq, n_bases = sc.codes_of(records)
    per_tile = np.bincount((rec_seq // T).astype(np.int64)) if n_bases else np.zeros(1, np.int64)
    if name.startswith(("many_small", "only_small")):
        assert per_tile.max() > CAP  # (the slice does not fit the LDS cap: searched in global memory)
    else:
        assert per_tile.max() + 1 <= CAP
    if name == "boundary_T":
        assert {T - 1, T, T + 1} <= set(rec_seq.tolist())
    if name == "reads150":
        assert n_bases % 16 != 0 and n_bases > T
    for canonical in (False, True):
        table = _half_table(records, k, canonical)
        want = _check(dev, records, k, table, canonical, twice=not canonical)
        total = want.sum(axis=0)
        if max(lengths) >= k + 1:
            assert total[1] > 0  # (hits)
            assert k < 21 or total[1] < total[0]  # (and windows that are none)
        if name in ("bases_k_minus_1", "two_short", "only_small"):
            assert total[0] == 0
    if name == "bases_k":
        rec = records[0][1]
        assert _check(dev, records, k, {rec: 3}).tolist() == [[1, 1, 3]]


@pytest.mark.parametrize("k", [4, 21, 32])
def test_n_runs_across_a_tile_boundary(dev, k):
    records = sc.n_run_records(k, T)
    for canonical in (False, True):
        table = sc.table_of(records[:1] + records[2:3], k, canonical)
        want = _check(dev, records, k, table, canonical)
        assert want[1].tolist() == [0, 0, 0]  # the all-N record
        assert 0 < want[0][0] < 2 * T + 77 - k + 1 and want[0][0] == want[0][1]
        assert want[2][0] == 90 - k + 1  # lower case is upper-cased


@functools.lru_cache(maxsize=None)
def _key_reads(k):
    records = sc.records_of([150] * 30 + [k, k + 1, 33], seed=k, prefix="read")
    if k % 2 == 0:
        pal = ("ACGT" * 8)[:k] if k % 4 == 0 else "AT" * (k // 2)
        assert sc.revcomp(pal) == pal
        records.append(("pal", "GG" + pal + "CA"))
    if k == 32:
        records += [("polyA", "A" * 40), ("polyT", "T" * 40), ("mixAT", "C" + "A" * 32 + "G" + "T" * 32)]
    return records


@pytest.mark.parametrize("canonical", [False, True])
@pytest.mark.parametrize("k", [2, 15, 16, 21, 31, 32])
def test_keys_and_tables(dev, k, canonical):
    records = _key_reads(k)
    names = [n for n, _ in records]
    all_t = sc.table_of(records, k, canonical)
    none_t = sc.table_of(sc.records_of([900], seed=77 + k, prefix="x"), k, canonical)
    half_t = _half_table(records, k, canonical)
    if k % 2 == 0:
        half_t.update({w: c for w, c in all_t.items() if w == sc.revcomp(w)})  # the palindromes are looked up
        assert any(w == sc.revcomp(w) for w in all_t)
    if k == 32:
        half_t.update({"A" * 32: 7} if canonical else {"A" * 32: 7, "T" * 32: 9})
        assert sc.key_of("T" * 32) == sc.MASK64 and sc.key_of("A" * 32) == 0
    want = _check(dev, records, k, all_t, canonical, twice=True)
    assert np.array_equal(want[:, 0], want[:, 1]) and want[:, 0].sum() > 0  # every window hits
    if k >= 15:
        assert _check(dev, records, k, none_t, canonical)[:, 1].sum() == 0
    want = _check(dev, records, k, half_t, canonical)
    if k >= 15:
        assert 0 < want[:, 1].sum() < want[:, 0].sum()
    if k == 32:
        a, t = want[names.index("polyA")], want[names.index("polyT")]
        assert a.tolist() == [9, 9, 63] and t.tolist() == ([9, 9, 63] if canonical else [9, 9, 81])
    empty = _check(dev, records, k, {}, canonical)  # nt == 0
    assert empty[:, 1:].sum() == 0 and np.array_equal(empty[:, 0], want[:, 0])
    # u64 counts above 2^32: the sum plane needs its upper word
    big_t = {w: c + (1 << 33) for w, c in half_t.items()}
    big = _check(dev, records, k, big_t, canonical, cb=8)
    assert int(big[:, 2].max()) > 1 << 33
    _check(dev, records, k, half_t, canonical, cb=8)
    # an explicit index width of 1 and of the maximum, next to the default
    for bits in (1, min(2 * k, MAXB)):
        _check(dev, records, k, half_t, canonical, bits=bits)


def test_refused_calls(dev):
    records = sc.records_of([150] * 3, seed=2)
    codes, rec_seq, n = sc.codes_of(records)
    keys, counts = sc.table_rows(sc.table_of(records, 9))
    bufs = [_up(dev, codes), _up(dev, rec_seq), _up(dev, keys), _up(dev, counts), dev.alloc(8 * 17)]
    fill = np.full(9 + PAD, SENT, np.uint64)
    out = _up(dev, fill)
    L = N.lib()
    try:
        d_codes, d_rec, d_keys, d_counts, d_index = bufs
        assert L.kman_table_index(dev.ctx, c_void_p(d_keys.ptr), len(keys), 9, 4, c_void_p(d_index.ptr)) == N.KMAN_OK

        def call(k=9, flags=0, cb=4, bits=4, n_bases=n, R=3):
            return L.kman_screen_records(dev.ctx, c_void_p(d_codes.ptr), n_bases, k, flags, c_void_p(d_rec.ptr), R,
                                         c_void_p(d_keys.ptr), c_void_p(d_counts.ptr), cb, len(keys),
                                         c_void_p(d_index.ptr), bits, c_void_p(out.ptr))

        for kw in (dict(k=1), dict(k=33), dict(flags=N.KMAN_RC), dict(flags=N.KMAN_CANONICAL | N.KMAN_MIXED),
                   dict(flags=N.KMAN_WANT_POS), dict(cb=2), dict(cb=16), dict(bits=0), dict(bits=19), dict(bits=25)):
            assert call(**kw) == N.KMAN_EINVAL, kw
        assert call(R=0) == N.KMAN_OK
        np.testing.assert_array_equal(dev.download(out, 9 + PAD, np.uint64), fill)  # nothing was written
        assert call(n_bases=8) == N.KMAN_OK  # fewer bases than k: no window, the planes are zero
        got = dev.download(out, 9 + PAD, np.uint64)
        assert np.all(got[:9] == 0) and np.all(got[9:] == SENT)
        assert call() == N.KMAN_OK  # the context is still usable
        got = dev.download(out, 9, np.uint64).reshape(3, 3).T
        np.testing.assert_array_equal(got, sc.stats(records, 9, sc.table_of(records, 9)))
    finally:
        for b in bufs + [out]:
            b.free()


# ----------------------------------------------------------------- engine API


def _engine_lines(dev, reads_text, table_text, k, canonical=False, fmt="auto", min_qual=0, index_bits=None,
                  keep_args=None):
    from kman_amd import engine

    p = engine.parse(dev, table_text)
    try:
        table = engine.join_groups(p, k, False, "count", canonical=canonical)
    finally:
        p.free()
    if table is None:
        table = engine.empty_count(dev, k)
    p = engine.parse(dev, reads_text, fmt, min_qual)
    try:
        st = engine.screen(p, table, canonical, index_bits=index_bits)
        assert st.shape == (p.n_records, 3) and st.dtype == np.uint64
        idx = engine.table_index(dev, table, index_bits)
        try:
            np.testing.assert_array_equal(engine.screen(p, table, canonical, index=idx, index_bits=index_bits), st)
        finally:
            idx.free()
        keep = None if keep_args is None else engine.screen_keep(st, *keep_args)
        return st, engine.emit_screen(p, st, keep)
    finally:
        p.free()
        engine.free_result(table)


@pytest.mark.parametrize("canonical", [False, True])
def test_engine_screen_fasta(dev, canonical):
    k = 21
    reads = sc.records_of([150] * 60 + [0, 20, 21, 0], seed=5, prefix="read")
    reads[3] = (reads[3][0], sc.with_n(reads[3][1], [(40, 44), (100, 101)]))
    genome = [("chr1", "".join(s for _, s in reads[::2])), ("chr2", sc.rand_seq(np.random.default_rng(6), 3000))]
    table = sc.table_of(genome, k, canonical)
    want = sc.stats(reads, k, table, canonical)
    assert 0 < want[:, 1].sum() < want[:, 0].sum()
    for bits, keep_args in ((None, None), (1, (1, 0.5, False)), (MAXB, (0, 0.9, True))):
        st, text = _engine_lines(dev, sc.fasta(reads), sc.fasta(genome), k, canonical, index_bits=bits,
                                 keep_args=keep_args)
        np.testing.assert_array_equal(st, want)
        kept = None if keep_args is None else sc.keep(want, *keep_args)
        assert text == sc.lines(reads, want, kept)
        if kept is not None:
            assert 0 < sum(kept) < len(reads)


@pytest.mark.parametrize("canonical, min_qual", [(False, 0), (True, 0), (False, 20), (True, 30)])
def test_engine_screen_fastq(dev, canonical, min_qual):
    import fastq_cases as fq
    from fastq_qual_cases import mask_fastq

    k = 11
    text = fq.mixed_reads(seed=3 + min_qual, n_records=120)
    fasta_text, n_masked = mask_fastq(text, min_qual, 33)
    assert (n_masked > 0) == (min_qual > 0)
    reads = sc.fasta_records(fasta_text)
    assert len(reads) >= 115 and any("\t" in n for n, _ in reads) and any(s == "" for _, s in reads)
    genome = [("g", "".join(s for _, s in sc.fasta_records(fq.fastq_to_fasta(text))[::3]))]
    table = sc.table_of(genome, k, canonical)
    want = sc.stats(reads, k, table, canonical)
    assert 0 < want[:, 1].sum() < want[:, 0].sum()
    st, out = _engine_lines(dev, text, sc.fasta(genome), k, canonical, "fastq", min_qual)
    np.testing.assert_array_equal(st, want)
    assert out == sc.lines(reads, want)


def test_engine_screen_refuses_word_keys(dev):
    from kman_amd import engine

    class _Table:
        k, n, count_bytes = 33, 0, 4

    with pytest.raises(AssertionError):
        engine.screen(None, _Table())
    with pytest.raises(AssertionError):
        engine.table_index(dev, _Table())


def test_hits_total_equals_match_counts(dev):
    """The existing kernel's answer to the same total: the counts of READS'
    distinct k-mers that are rows of the table (match_counts, "left")."""
    from kman_amd import engine

    k = 17
    reads = sc.records_of([150] * 80, seed=12, prefix="read")
    genome = [("g", "".join(s for _, s in reads[::2]) + sc.rand_seq(np.random.default_rng(13), 2000))]
    pt = engine.parse(dev, sc.fasta(genome))
    try:
        table = engine.join_groups(pt, k, False, "count")
    finally:
        pt.free()
    p = engine.parse(dev, sc.fasta(reads))
    ra = v = None
    try:
        st = engine.screen(p, table)
        ra = engine.join_groups(p, k, False, "count")
        v = engine.match_counts(dev, ra, table, "left")
        left = dev.download(v, ra.n, np.uint32 if 8 not in (ra.count_bytes, table.count_bytes) else np.uint64)
        assert int(st[:, 1].sum()) == int(left.sum()) > 0
        assert int(st[:, 0].sum()) == 80 * (150 - k + 1) > int(st[:, 1].sum())
    finally:
        p.free()
        if v is not None:
            v.free()
        engine.free_result(ra)
        engine.free_result(table)


# ------------------------------------------------------------------------ CLI


def _cli(*argv):
    from kman_amd.scripts.kmer import main

    r = CliRunner().invoke(main, [str(a) for a in argv], catch_exceptions=False)
    assert r.exit_code == 0, r.output


def test_cli_end_to_end(tmp_path):
    import fastq_cases as fq

    k = 21
    reads = sc.records_of([150] * 50 + [10, 0, 21], seed=21, prefix="read")
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
        assert 0 < want[:, 1].sum() < want[:, 0].sum()
        _cli("screen", tmp_path / "reads.fa", tmp_path / "genome.fa", out, k, *flags)
        assert out.read_bytes() == sc.lines(reads, want)
        assert out.read_bytes().count(b"\n") == len(reads)  # one line per read
        # only the solid k-mers of the table are looked up
        solid = sc.table_of(genome, k, canonical, min_count=2)
        assert 0 < len(solid) < len(table)
        want2 = sc.stats(reads, k, solid, canonical)
        _cli("screen", tmp_path / "reads.fa", tmp_path / "genome.fa", out, k, "-L", 2, *flags)
        assert out.read_bytes() == sc.lines(reads, want2)
        _cli("screen", tmp_path / "reads.fa", tmp_path / "genome.fa", out, k, "-L", 2, "-U", 2, "--index-bits", 3,
             *flags)
        assert out.read_bytes() == sc.lines(reads, sc.stats(reads, k, sc.table_of(genome, k, canonical, 2, 2),
                                                            canonical))
        for argv, ka in ((["--min-hits", 1], (1, 0.0, False)), (["--min-frac", 0.5], (0, 0.5, False)),
                         (["--min-hits", 100, "--min-frac", 1.0, "-v"], (100, 1.0, True)),
                         (["--min-hits", 1, "--invert"], (1, 0.0, True))):
            kept = sc.keep(want, *ka)
            assert 0 < sum(kept) < len(reads)
            _cli("screen", tmp_path / "reads.fa", tmp_path / "genome.fa", out, k, *argv, *flags)
            assert out.read_bytes() == sc.lines(reads, want, kept), argv
    # FASTQ reads against a gzipped FASTA, with a quality threshold on the reads
    from fastq_qual_cases import mask_fastq

    text = fq.mixed_reads(seed=8, n_records=80)
    (tmp_path / "reads.fq").write_bytes(text)
    k = 9
    fq_reads = sc.fasta_records(fq.fastq_to_fasta(text))
    genome = [("g", "".join(s for _, s in fq_reads[::2]))]
    with gzip.open(tmp_path / "g.fa.gz", "wb") as fh:
        fh.write(sc.fasta(genome))
    table = sc.table_of(genome, k)
    for q in (0, 25):
        masked = sc.fasta_records(mask_fastq(text, q, 33)[0])
        want = sc.stats(masked, k, table)
        assert 0 < want[:, 1].sum() < want[:, 0].sum()
        _cli("screen", tmp_path / "reads.fq", tmp_path / "g.fa.gz", out, k, *(["-q", q] if q else []))
        assert out.read_bytes() == sc.lines(masked, want), q


def test_cli_empty_table_and_reads_without_windows(tmp_path):
    k = 21
    reads = sc.records_of([150] * 5 + [0, 30], seed=31, prefix="read")
    (tmp_path / "reads.fa").write_bytes(sc.fasta(reads))
    (tmp_path / "none.fa").write_bytes(b">x\nACGTACG\n>y\nNNNNNNNNNNNNNNNNNNNNNNNNNNNNNN\n")
    out = tmp_path / "out.tsv"
    # a table input without k-mers: every line shows 0 hits
    _cli("screen", tmp_path / "reads.fa", tmp_path / "none.fa", out, k)
    want = sc.stats(reads, k, {})
    assert want[:, 0].sum() > 0 and want[:, 1:].sum() == 0
    assert out.read_bytes() == sc.lines(reads, want)
    # READS with no valid window at all
    none = sc.fasta_records(b">x\nACGTACG\n>y\nNNNNNNNNNNNNNNNNNNNNNNNNNNNNNN\n")
    _cli("screen", tmp_path / "none.fa", tmp_path / "reads.fa", out, k)
    assert out.read_bytes() == b"x\t0\t0\t0\ny\t0\t0\t0\n" == sc.lines(none, sc.stats(none, k, sc.table_of(reads, k)))
    _cli("screen", tmp_path / "none.fa", tmp_path / "reads.fa", out, k, "--min-hits", 1)
    assert out.read_bytes() == b""
    with pytest.raises(AssertionError, match="K <= 32"):
        _cli("screen", tmp_path / "reads.fa", tmp_path / "reads.fa", tmp_path / "no.tsv", 33)
    assert not (tmp_path / "no.tsv").exists()
