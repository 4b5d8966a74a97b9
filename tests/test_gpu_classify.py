"""Reads among references on the GPU: kman_classify_records, kman_classify_pick,
engine.color_table / classify and `kmer classify` against the plain-Python
statement (tests/classify_cases.py), all for equality."""

from __future__ import annotations

import functools
import gzip
from ctypes import c_void_p

import numpy as np
import pytest
from click.testing import CliRunner

import classify_cases as cc
import reads_cases as rcs
import screen_cases as sc

pytestmark = pytest.mark.gpu

from kman_amd import _native as N  # noqa: E402

T = N.KMAN_SCREEN_TILE
CAP = N.KMAN_SCREEN_REC_CAP
MAXB = N.KMAN_SCREEN_MAX_INDEX_BITS
SPEC = N.KMAN_CLASSIFY_SPECIFIC
PAD = 16  # sentinel words after an output
SENT = 0xA5A5A5A5


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


# ------------------------------------------------------ kman_classify_records


def _classify(dev, records, k, ctable, nc, canonical=False, specific=False, bits=None, twice=False):
    """kman_classify_records on the helper's device layout of `records`, the
    output pre-filled with a nonzero pattern; the (1 + nc, n_records) result."""
    from kman_amd import engine

    codes, rec_seq, n_bases = sc.codes_of(records)
    keys, masks = cc.table_rows(ctable)
    R = len(records)
    if bits is None:
        bits = engine.default_index_bits(len(keys), k)
    L = N.lib()
    flags = (N.KMAN_CANONICAL if canonical else 0) | (SPEC if specific else 0)
    bufs = [_up(dev, codes), _up(dev, rec_seq), _up(dev, keys), _up(dev, masks), dev.alloc(8 * ((1 << bits) + 1)), None]
    try:
        d_codes, d_rec, d_keys, d_masks, d_index, _ = bufs
        assert L.kman_table_index(dev.ctx, c_void_p(d_keys.ptr), len(keys), k, bits, c_void_p(d_index.ptr)) == N.KMAN_OK
        words = (1 + nc) * R
        fill = np.full(words + PAD, SENT, np.uint32)
        runs = []
        for _ in range(2 if twice else 1):
            d_out = bufs[5] = _up(dev, fill)
            rc = L.kman_classify_records(dev.ctx, c_void_p(d_codes.ptr), n_bases, k, flags, c_void_p(d_rec.ptr), R,
                                         c_void_p(d_keys.ptr), c_void_p(d_masks.ptr), len(keys),
                                         c_void_p(d_index.ptr), bits, nc, c_void_p(d_out.ptr))
            assert rc == N.KMAN_OK, L.kman_last_error(dev.ctx)
            got = dev.download(d_out, words + PAD, np.uint32)
            d_out.free()
            bufs[5] = None
            assert np.all(got[words:] == SENT)  # nothing past the planes
            runs.append(got[:words])
        if twice:
            assert runs[0].tobytes() == runs[1].tobytes()  # the same call twice: identical bytes
        np.testing.assert_array_equal(dev.download(d_rec, R, np.uint64), rec_seq)  # (inputs are not written)
        return runs[0].reshape(1 + nc, R)
    finally:
        for b in bufs:
            if b is not None:
                b.free()


def _check(dev, records, k, ctable, nc, canonical=False, specific=False, bits=None, twice=False):
    want = cc.planes(records, k, ctable, nc, canonical, specific)
    got = _classify(dev, records, k, ctable, nc, canonical, specific, bits, twice)
    np.testing.assert_array_equal(got, want)
    return want


def _refs(records, nc, seed, full=True):
    """nc references: random overlapping substrings of the reads; with `full`
    the LAST one holds every read (bit nc - 1 is on every row) and, from three
    references on, the second one is empty."""
    refs = cc.substring_refs(records, nc, seed)
    if full and nc >= 2:
        refs[nc - 1] = list(records)
    if nc >= 3:
        refs[1] = []
    return refs


LAYOUTS = sorted(sc.layouts(5, T, CAP)) + ["n_runs"]


@pytest.mark.parametrize("name", LAYOUTS)
def test_record_layouts_nine_colours(dev, name):
    """Every record layout of the screen tests at one colour past a chunk."""
    k, nc = 21, 9
    if name == "n_runs":
        records = sc.n_run_records(k, T)
    else:
        records = sc.records_of(sc.layouts(k, T, CAP)[name], seed=len(name) + k)
    _, rec_seq, n_bases = sc.codes_of(records)
    per_tile = np.bincount((rec_seq // T).astype(np.int64)) if n_bases else np.zeros(1, np.int64)
    if name.startswith(("many_small", "only_small")):
        assert per_tile.max() > CAP  # (the slice does not fit the LDS cap: searched in global memory)
    else:
        assert per_tile.max() + 1 <= CAP
    has_kmers = any(len(s) >= k + 8 for _, s in records)
    for canonical in (False, True):
        refs = _refs(records, nc, seed=len(name), full=not canonical) if has_kmers else [list(records)] * nc
        ct = cc.color_table_of(refs, k, canonical)
        want = _check(dev, records, k, ct, nc, canonical, twice=not canonical)
        spec = _check(dev, records, k, ct, nc, canonical, specific=True)
        if has_kmers:
            assert want[1:].sum() > 0 and want[2].sum() == 0  # hits; the empty reference has none
            assert want[9].sum() > 0  # the colour of the second chunk
            assert np.all(spec[1:] <= want[1:]) and spec[1:].sum() < want[1:].sum()
            if not canonical:
                assert np.array_equal(want[9], want[0])  # the reference that holds every read
        if name in ("bases_k_minus_1", "two_short", "only_small"):
            assert want.sum() == 0


@functools.lru_cache(maxsize=None)
def _sweep_records(name, k):
    records = sc.records_of(sc.layouts(k, T, CAP)[name], seed=len(name) + k, prefix="read")
    if k == 32:
        records = records + [("polyA", "A" * 40), ("polyT", "T" * 40), ("mixAT", "C" + "A" * 32 + "G" + "T" * 32)]
    return records


@pytest.mark.parametrize("k", [3, 21, 32])
@pytest.mark.parametrize("name", ["reads150", "spanning", "many_small_carry", "boundary_T"])
def test_colour_sweep(dev, name, k):
    records = _sweep_records(name, k)
    names = [n for n, _ in records]
    for nc in (1, 2, 8, 33, 64):
        for full in ((True, False) if nc in (1, 64) else (nc == 33,)):
            refs = _refs(records, nc, seed=nc + k, full=full)
            if k == 32:
                refs[0] = refs[0] + [("pa", "A" * 33), ("pt", "T" * 32)]  # keys 0 and 2^64 - 1
            for canonical in ((False, True) if nc in (1, 64) else (nc == 8,)):
                ct = cc.color_table_of(refs, k, canonical)
                if k == 32:
                    assert ct["A" * 32] & 1 and (canonical or ct["T" * 32] & 1)
                for specific in ((False, True) if nc in (1, 64) or full is False else (False,)):
                    want = _check(dev, records, k, ct, nc, canonical, specific)
                    assert want[0].sum() > 0
                    if not specific or nc == 1:
                        assert want[1].sum() > 0
                    if full and nc >= 2 and not specific:
                        assert np.array_equal(want[nc], want[0])  # bit nc - 1 (bit 63 at nc = 64): every window
                    if k == 32 and not specific:
                        a, t = want[:, names.index("polyA")], want[:, names.index("polyT")]
                        assert a[0] == 9 and a[1] == 9 and t[0] == 9 and t[1] == 9
    # index widths 1 and the widest, next to the default
    refs = _refs(records, 9, seed=k)
    ct = cc.color_table_of(refs, k)
    for bits in (1, min(2 * k, MAXB)):
        _check(dev, records, k, ct, 9, bits=bits)


def test_mask_bits_at_or_above_n_colors_are_ignored(dev):
    k = 21
    records = sc.records_of([150] * 40 + [37], seed=4)
    ct = cc.color_table_of(_refs(records, 64, seed=8), k)
    some = sorted(ct)[::7]
    for w in some:
        ct[w] = (1 << 64) - 1  # an all-ones mask
    assert max(ct.values()) == (1 << 64) - 1 and any(m >> 9 and m != (1 << 64) - 1 for m in ct.values())
    for nc in (1, 7, 8, 9, 63):
        cut = {w: m & ((1 << nc) - 1) for w, m in ct.items()}
        cut = {w: m for w, m in cut.items() if m}
        for specific in (False, True):
            want = cc.planes(records, k, cut, nc, specific=specific)
            np.testing.assert_array_equal(cc.planes(records, k, ct, nc, specific=specific), want)
            np.testing.assert_array_equal(_classify(dev, records, k, ct, nc, specific=specific), want)
            np.testing.assert_array_equal(_classify(dev, records, k, cut, nc, specific=specific), want)
            assert want[1:].sum() > 0
    # rows whose mask is 0 are rows nobody holds
    zero = dict(ct)
    for w in some:
        zero[w] = 0
    want = _check(dev, records, k, zero, 9)
    assert 0 < want[1:].sum()


def test_empty_table_short_inputs_and_refused_calls(dev):
    k = 9
    records = sc.records_of([150] * 3, seed=2)
    codes, rec_seq, n = sc.codes_of(records)
    ct = cc.color_table_of([records[:1], records[1:]], k)
    keys, masks = cc.table_rows(ct)
    nc = 2
    words = (1 + nc) * 3
    bufs = [_up(dev, codes), _up(dev, rec_seq), _up(dev, keys), _up(dev, masks), dev.alloc(8 * 17)]
    odd = _up(dev, np.concatenate([np.zeros(8, np.uint8), codes]))  # the codes off 16-byte alignment
    fill = np.full(65 * 3 + PAD, SENT, np.uint32)
    out = _up(dev, fill)
    L = N.lib()
    try:
        d_codes, d_rec, d_keys, d_masks, d_index = bufs
        assert L.kman_table_index(dev.ctx, c_void_p(d_keys.ptr), len(keys), k, 4, c_void_p(d_index.ptr)) == N.KMAN_OK

        def call(k=k, flags=0, bits=4, n_bases=n, R=3, nc=nc, nt=len(keys), codes_ptr=d_codes.ptr):
            return L.kman_classify_records(dev.ctx, c_void_p(codes_ptr), n_bases, k, flags, c_void_p(d_rec.ptr), R,
                                           c_void_p(d_keys.ptr), c_void_p(d_masks.ptr), nt, c_void_p(d_index.ptr),
                                           bits, nc, c_void_p(out.ptr))

        for kw in (dict(k=1), dict(k=33), dict(flags=N.KMAN_RC), dict(flags=N.KMAN_CANONICAL | N.KMAN_MIXED),
                   dict(flags=N.KMAN_WANT_POS), dict(flags=SPEC | 32), dict(nc=0), dict(nc=65), dict(bits=0),
                   dict(bits=19), dict(bits=25), dict(codes_ptr=odd.ptr + 8)):
            assert call(**kw) == N.KMAN_EINVAL, kw
        assert call(R=0) == N.KMAN_OK
        np.testing.assert_array_equal(dev.download(out, len(fill), np.uint32), fill)  # nothing was written
        want = cc.planes(records, k, ct, nc)
        # fewer bases than k: no window, the planes are zero (exactly k bases: the layout "bases_k" above)
        assert call(n_bases=k - 1) == N.KMAN_OK
        got = dev.download(out, len(fill), np.uint32)
        assert np.all(got[:words] == 0) and np.all(got[words:] == SENT)
        dev.upload(out, fill)
        assert call(nt=0) == N.KMAN_OK  # an empty table: the windows are counted, nothing hits
        got = dev.download(out, words, np.uint32).reshape(1 + nc, 3)
        assert np.array_equal(got[0], want[0]) and got[1:].sum() == 0
        assert call() == N.KMAN_OK  # the context is still usable
        np.testing.assert_array_equal(dev.download(out, words, np.uint32).reshape(1 + nc, 3), want)
        assert call(flags=SPEC | N.KMAN_CANONICAL) == N.KMAN_OK
    finally:
        for b in bufs + [out, odd]:
            b.free()


# --------------------------------------------------------- kman_classify_pick


def _pick(dev, hit_planes, nc=None):
    hp = np.ascontiguousarray(hit_planes, dtype=np.uint32)
    nc = hp.shape[0] if nc is None else nc
    R = hp.shape[1]
    planes = np.concatenate([np.full(R, 0x12345678, np.uint32), hp.reshape(-1)])  # (plane 0 is not read)
    d_in = _up(dev, planes)
    fill = np.full(3 * R + PAD, SENT, np.uint32)
    d_out = _up(dev, fill)
    try:
        rc = N.lib().kman_classify_pick(dev.ctx, c_void_p(d_in.ptr), R, nc, c_void_p(d_out.ptr))
        got = dev.download(d_out, 3 * R + PAD, np.uint32)
        assert np.all(got[3 * R:] == SENT)
        return rc, got[:3 * R].reshape(3, R)
    finally:
        d_in.free()
        d_out.free()


def test_pick_on_hand_made_planes(dev):
    top = (1 << 32) - 1
    # columns: all zero | max first | max in the middle | max last | two-way tie | three-way tie | 2^32 - 1 twice
    #          | 2^32 - 1 once
    hp = np.asarray([[0, 9, 1, 0, 5, 7, top, 3],
                     [0, 2, 8, 1, 0, 7, 1, top],
                     [0, 3, 2, 2, 5, 0, top, top - 1],
                     [0, 1, 0, 6, 4, 7, 0, 0]], dtype=np.uint32)
    rc, got = _pick(dev, hp)
    assert rc == N.KMAN_OK
    np.testing.assert_array_equal(got, cc.pick(hp))
    assert got.tolist() == [[cc.NONE, 0, 1, 3, 0, 0, 0, 1], [0, 9, 8, 6, 5, 7, top, top],
                            [0, 3, 2, 2, 5, 7, top, top - 1]]
    rc, got = _pick(dev, hp[:1])  # one colour: no runner-up
    assert rc == N.KMAN_OK and got.tolist() == [[cc.NONE, 0, 0, cc.NONE, 0, 0, 0, 0], hp[0].tolist(), [0] * 8]
    rc, got = _pick(dev, hp[:, 3:4])  # one record
    assert rc == N.KMAN_OK and got.tolist() == [[3], [6], [2]]
    rng = np.random.default_rng(3)
    for nc, R in ((64, 1000), (64, 1), (2, 1000), (33, 257)):
        hp = rng.integers(0, 6, (nc, R)).astype(np.uint32)  # small values: many ties, many zeros
        hp[:, ::5] = rng.integers(0, 1 << 32, hp[:, ::5].shape, dtype=np.uint64).astype(np.uint32)
        hp[nc - 1, 7 % R] = top  # the maximum in the last colour
        rc, got = _pick(dev, hp)
        assert rc == N.KMAN_OK
        np.testing.assert_array_equal(got, cc.pick(hp))
    for nc in (0, 65):  # refused: nothing written
        rc, got = _pick(dev, hp, nc=nc)
        assert rc == N.KMAN_EINVAL and np.all(got == SENT)


# ----------------------------------------------------------------- engine API


def _count_table(dev, records, k, canonical=False):
    from kman_amd import engine

    if not records:
        return engine.empty_count(dev, k)
    p = engine.parse(dev, sc.fasta(records))
    try:
        t = engine.join_groups(p, k, False, "count", canonical=canonical)
    finally:
        p.free()
    return t if t is not None else engine.empty_count(dev, k)


def _color_table(dev, refs, k, canonical=False):
    from kman_amd import engine

    tables = [_count_table(dev, r, k, canonical) for r in refs]
    try:
        return engine.color_table(dev, tables)
    finally:
        for t in tables:
            engine.free_result(t)


def test_color_table(dev):
    from kman_amd import engine

    k = 11
    rng = np.random.default_rng(17)
    a = [("a", sc.rand_seq(rng, 700))]
    b = [("b", a[0][1][300:600] + sc.rand_seq(rng, 300))]
    c = [("c", sc.rand_seq(rng, 500)), ("c2", a[0][1][:100])]
    d = [("d", sc.rand_seq(rng, 400))]  # disjoint from the others at k = 11, nearly surely; checked below
    none = [("n", "ACGT")]  # no 11-mer: an empty table
    many = [[("m%d" % i, (a[0][1] + b[0][1] + c[0][1])[7 * i:7 * i + 60])] for i in range(64)]
    cases = {
        "one": [a], "two": [a, b], "three": [a, b, c], "identical": [a, a], "disjoint": [a, d],
        "empty_first": [none, a, b], "empty_middle": [a, none, b], "empty_last": [a, b, none],
        "all_empty": [none, []], "sixty_four": many,
    }
    assert not set(sc.table_of(a, k)) & set(sc.table_of(d, k))
    for name, refs in cases.items():
        for canonical in ((False, True) if name in ("three", "sixty_four") else (False,)):
            want = cc.color_table_of(refs, k, canonical)
            wk, wm = cc.table_rows(want)
            ct = _color_table(dev, refs, k, canonical)
            try:
                assert ct.count_bytes == 8 and ct.k == k and ct.n == len(wk), name
                keys = dev.download(ct.ukeys, ct.n, np.uint64)
                masks = dev.download(ct.counts, ct.n, np.uint64)
            finally:
                engine.free_result(ct)
            assert np.all(keys[1:] > keys[:-1]), name  # strictly ascending
            np.testing.assert_array_equal(keys, wk, err_msg=name)
            np.testing.assert_array_equal(masks, wm, err_msg=name)
            if name == "sixty_four":
                assert int(masks.max()) >> 63 == 1 and any(bin(int(m)).count("1") > 3 for m in masks)
            if name == "identical":
                assert set(masks.tolist()) == {3}
            if name == "disjoint":
                assert set(masks.tolist()) == {1, 2}
    ta, tb = _count_table(dev, a, k), _count_table(dev, a, k + 1)
    try:
        with pytest.raises(AssertionError):
            engine.color_table(dev, [ta, tb])  # mixed k
        with pytest.raises(AssertionError):
            engine.color_table(dev, [])
        with pytest.raises(AssertionError):
            engine.color_table(dev, [ta] * 65)
    finally:
        engine.free_result(ta)
        engine.free_result(tb)


@pytest.mark.parametrize("layout", ["reads150", "spanning"])
def test_engine_classify_and_the_screen_of_each_reference(dev, layout):
    """engine.classify against the statement, and, without `specific`, the
    hit column of reference c against engine.screen's HITS for c's own table."""
    from kman_amd import engine

    k = 21
    reads = sc.records_of(sc.layouts(k, T, CAP)[layout], seed=11, prefix="read")
    refs = cc.substring_refs(reads, 3, seed=5, pieces=6, length=140)
    labels = ["x", "y", "z"]
    p = engine.parse(dev, sc.fasta(reads))
    try:
        for canonical in (False, True):
            ctd = cc.color_table_of(refs, k, canonical)
            ct = _color_table(dev, refs, k, canonical)
            try:
                for specific in (False, True):
                    want = cc.planes(reads, k, ctd, 3, canonical, specific)
                    wpk = cc.pick(want[1:])
                    w, best, hits, second, pl = engine.classify(p, ct, 3, canonical, specific, planes=True)
                    for arr in (w, best, hits, second, pl):
                        assert arr.dtype == np.uint32
                    np.testing.assert_array_equal(w, want[0])
                    np.testing.assert_array_equal(pl, want[1:].T)
                    np.testing.assert_array_equal(np.stack([best, hits, second]), wpk)
                    idx = engine.table_index(dev, ct, 5)
                    try:
                        four = engine.classify(p, ct, 3, canonical, specific, index=idx, index_bits=5)
                    finally:
                        idx.free()
                    assert len(four) == 4
                    np.testing.assert_array_equal(np.stack(four), np.concatenate([want[:1], wpk]))
                    a = engine.classify_assign(w, best, hits, second)
                    wa = cc.assign(want[0], wpk[0], wpk[1], wpk[2])
                    assert a.tolist() == wa
                    assert engine.emit_classify(p, labels, w, a, hits, second) == \
                        cc.lines(reads, labels, want[0], wa, wpk[1], wpk[2])
                    assert engine.emit_classify(p, labels, w, a, hits, second, planes=pl) == \
                        cc.lines(reads, labels, want[0], wa, wpk[1], wpk[2], want[1:])
                    if not specific:
                        assert pl.sum() > 0
                        for c in range(3):
                            t = _count_table(dev, refs[c], k, canonical)
                            try:
                                st = engine.screen(p, t, canonical)
                            finally:
                                engine.free_result(t)
                            np.testing.assert_array_equal(st[:, 0], w.astype(np.uint64))
                            np.testing.assert_array_equal(st[:, 1], pl[:, c].astype(np.uint64))
            finally:
                engine.free_result(ct)
    finally:
        p.free()


def test_engine_classify_refuses(dev):
    from kman_amd import engine

    class _Table:
        k, n, count_bytes = 33, 0, 8

    class _Narrow:
        k, n, count_bytes = 21, 0, 4

    with pytest.raises(AssertionError):
        engine.classify(None, _Table(), 2)
    with pytest.raises(AssertionError):
        engine.classify(None, _Narrow(), 2)
    for nc in (0, 65, True, 1.5):
        _Narrow.count_bytes = 8
        with pytest.raises(AssertionError):
            engine.classify(None, _Narrow(), nc)


# ------------------------------------------------------------------------ CLI


def _cli(*argv):
    from kman_amd.scripts.kmer import main

    r = CliRunner().invoke(main, [str(a) for a in argv], catch_exceptions=False)
    assert r.exit_code == 0, r.output


def _three_refs(reads, seed):
    """Three references over the reads' sequences: each holds a third of the
    reads whole, all hold the first six (shared k-mers), and each repeats one
    stretch (k-mers with a count of 2 inside the reference, for -L 2)."""
    rng = np.random.default_rng(seed)
    seqs = [s for _, s in reads if len(s) >= 60]
    refs = []
    for c in range(3):
        own = "N".join(seqs[c::3][:12])
        shared = "N".join(seqs[:6])
        refs.append([("chr%d" % c, own), ("shared%d" % c, shared), ("dup%d" % c, seqs[c][:50]),
                     ("junk%d" % c, sc.rand_seq(rng, 300))])
    return refs


def _check_run(tmp, reads_path, reads, text, offsets, ext, refs, ref_paths, k, argv=(), **kw):
    labels = [cc.label_of(str(p)) for p in ref_paths]
    pl, pk, a, kmers = cc.classify(reads, labels, refs, k, **kw)
    out, summ, pre = tmp / "out.tsv", tmp / "summary.tsv", tmp / "cut"
    ref_args = [x for p in ref_paths for x in ("--ref", p)]
    _cli("classify", reads_path, out, k, *ref_args, "--summary", summ, "--reads-out-prefix", pre, *argv)
    assert out.read_bytes() == cc.lines(reads, labels, pl[0], a, pk[1], pk[2])
    assert out.read_bytes().count(b"\n") == len(reads)  # one line per read
    assert summ.read_bytes() == cc.summary(labels, kmers, a)
    files = cc.cut_files(text, offsets, labels, a, str(pre), ext)
    assert len(files) == len(labels) + 2
    for path, want in files.items():
        with open(path, "rb") as fh:
            assert fh.read() == want, path
    _cli("classify", reads_path, out, k, *ref_args, "--hits", *argv)
    assert out.read_bytes() == cc.lines(reads, labels, pl[0], a, pk[1], pk[2], pl[1:])
    return a


def test_cli_end_to_end(tmp_path):
    import fastq_cases as fq
    from fastq_qual_cases import mask_fastq

    k = 21
    reads = sc.records_of([150] * 60 + [10, 0, 21], seed=21, prefix="read")
    refs = _three_refs(reads, seed=22)
    text = sc.fasta(reads)
    (tmp_path / "reads.fa").write_bytes(text)
    paths = [tmp_path / "human.fa", tmp_path / "mouse.fasta.gz", tmp_path / "vector"]
    paths[0].write_bytes(sc.fasta(refs[0]))
    with gzip.open(paths[1], "wb") as fh:
        fh.write(sc.fasta(refs[1]))
    paths[2].write_bytes(sc.fasta(refs[2]))
    assert [cc.label_of(str(p)) for p in paths] == ["human", "mouse", "vector"]
    off = rcs.fasta_offsets(text)
    seen = set()
    for argv, kw in (([], {}), (["--canonical"], dict(canonical=True)), (["--specific"], dict(specific=True)),
                     (["--canonical", "--specific"], dict(canonical=True, specific=True)),
                     (["--canonical", "-L", 2], dict(canonical=True, min_count=2)),
                     (["--min-margin", 40, "--min-frac", 0.3, "--index-bits", 3], dict(min_margin=40, min_frac=0.3)),
                     (["--min-hits", 200], dict(min_hits=200))):
        a = _check_run(tmp_path, tmp_path / "reads.fa", reads, text, off, "fa", refs, paths, k, argv, **kw)
        seen.update(a)
        if argv == ["--min-hits", 200]:
            assert set(a) == {-1}  # every read is unassigned
        if argv == ["--canonical", "-L", 2]:
            assert 0 in a or 1 in a or 2 in a
    assert seen == {-2, -1, 0, 1, 2}
    # one --ref
    a = _check_run(tmp_path, tmp_path / "reads.fa", reads, text, off, "fa", refs[:1], paths[:1], k)
    assert set(a) == {-1, 0}
    # gzipped FASTQ reads with a quality threshold
    k = 9
    qtext = fq.mixed_reads(seed=8, n_records=80)
    with gzip.open(tmp_path / "reads.fq.gz", "wb") as fh:
        fh.write(qtext)
    plain = sc.fasta_records(fq.fastq_to_fasta(qtext))
    qrefs = [[("g%d" % c, "N".join(s for _, s in plain[c::3][:10]))] for c in range(3)]
    qpaths = [tmp_path / ("q%d.fa" % c) for c in range(3)]
    for path, r in zip(qpaths, qrefs):
        path.write_bytes(sc.fasta(r))
    qoff = rcs.fastq_offsets(qtext)
    for q in (0, 25):
        masked = sc.fasta_records(mask_fastq(qtext, q, 33)[0])
        a = _check_run(tmp_path, tmp_path / "reads.fq.gz", masked, qtext, qoff, "fq", qrefs, qpaths, k,
                       ["-q", q] if q else [])
        assert len(set(a)) >= 3
