"""All pairs of a coloured table on the GPU: kman_mask_gram, engine.mask_gram
and `kmer compare` against the plain-Python statement (tests/compare_cases.py),
all for equality."""

from __future__ import annotations

import gzip
from ctypes import c_void_p

import numpy as np
import pytest
from click.testing import CliRunner

import classify_cases as cc
import compare_cases as cmp
import hpc_cases as hc
import screen_cases as sc

pytestmark = pytest.mark.gpu

from kman_amd import _native as N  # noqa: E402

PAD = 16  # sentinel words after an output
SENT = 0xA5A5A5A5A5A5A5A5
STRIDE = N.KMAN_GRAM_MAX_BLOCKS * N.KMAN_GRAM_THREADS  # rows of one full grid stride (include/kman.h)
SMALL_N = (0, 1, 63, 64, 65, 255, 256, 257)  # a wave's edge, a block's edge
BIG_N = STRIDE + 64 + 1  # one wave more than a full grid stride, and one row
COLORS = (1, 2, 11, 33, 63, 64)
KINDS = ("ones", "zero", "one_bit", "dense", "sparse", "garbage")


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


def _gram(dev, masks, nc, occ=True, private=True, shift=0, twice=False, rc_want=None, gram=True, n=None):
    """kman_mask_gram on `masks` (uploaded `shift` bytes into their buffer),
    every output pre-filled with a sentinel pattern and followed by PAD sentinel
    words.  Returns (rc, G, occ, private); an output that was not passed is
    None.  A refused call must leave every sentinel intact."""
    masks = np.ascontiguousarray(masks, dtype=np.uint64)
    n = len(masks) if n is None else n
    ncw = max(1, min(nc, 64))  # (sizes of the buffers of a call that is refused for its n_colors)
    sizes = (ncw * ncw, ncw + 1, ncw)
    d_masks = dev.alloc(max(16, masks.nbytes + 16))
    bufs = [d_masks]
    try:
        if masks.nbytes:
            dev.upload(d_masks, masks, shift)
        runs = []
        for _ in range(2 if twice else 1):
            outs = [_up(dev, np.full(w + PAD, SENT, np.uint64)) for w in sizes]
            bufs += outs
            ptrs = [c_void_p(b.ptr) if use else None for b, use in zip(outs, (gram, occ, private))]
            rc = N.lib().kman_mask_gram(dev.ctx, c_void_p(d_masks.ptr + shift), n, nc, *ptrs)
            got = [dev.download(b, w + PAD, np.uint64) for b, w in zip(outs, sizes)]
            for b in outs:
                b.free()
                bufs.remove(b)
            if rc_want is not None:
                assert rc == rc_want
            else:
                assert rc == N.KMAN_OK, N.lib().kman_last_error(dev.ctx)
            res = []
            for g, w, use in zip(got, sizes, (gram, occ, private)):
                assert np.all(g[w:] == SENT)  # nothing past the output
                if rc != N.KMAN_OK or not use:
                    assert np.all(g == SENT)  # a refused call, or a NULL output: nothing written
                    res.append(None)
                else:
                    res.append(g[:w])
            runs.append(res)
        if twice:
            for x, y in zip(*runs):
                assert x.tobytes() == y.tobytes()  # the same call twice: identical bytes
        if masks.nbytes:
            np.testing.assert_array_equal(dev.download(d_masks, len(masks), np.uint64, shift), masks)  # not written
        G, o, p = runs[0]
        return rc, (G.reshape(ncw, ncw) if G is not None else None), o, p
    finally:
        for b in bufs:
            b.free()


def _check(dev, masks, nc, **kw):
    wG, wo, wp = cmp.as_arrays(*cmp.mask_gram(masks, nc))
    _, G, o, p = _gram(dev, masks, nc, **kw)
    np.testing.assert_array_equal(G, wG)
    np.testing.assert_array_equal(o, wo)
    np.testing.assert_array_equal(p, wp)
    return wG, wo, wp


def _identities(G, occ, private, n):
    G, occ, private = (np.asarray(x, dtype=object) for x in (G, occ, private))
    assert np.array_equal(G, G.T)
    assert int(occ.sum()) == n
    assert sum(p * int(occ[p]) for p in range(len(occ))) == int(np.trace(G))
    assert all(int(private[c]) <= int(G[c][c]) for c in range(len(private)))


@pytest.mark.parametrize("nc", COLORS)
def test_row_counts_and_mask_kinds(dev, nc):
    for n in SMALL_N:
        cases = cmp.mask_cases(n, nc, seed=100 * nc + n)
        assert sorted(cases) == sorted(KINDS)
        for kind in KINDS:
            G, occ, private = _check(dev, cases[kind], nc, twice=kind == "dense")
            _identities(G, occ, private, n)
            if kind == "zero":
                assert int(occ[0]) == n and not G.any()
            if kind == "ones":
                assert np.all(G == n) and int(occ[nc]) == n
            if kind == "one_bit":
                assert not (G - np.diag(np.diag(G))).any() and int(private.sum()) == n and int(occ[1]) == n
            if kind == "garbage" and n:
                cut = cases[kind] & np.uint64((1 << nc) - 1)
                got = _gram(dev, cut, nc)  # the cut masks give the same result
                np.testing.assert_array_equal(got[1], G)
                np.testing.assert_array_equal(got[2], occ)
                np.testing.assert_array_equal(got[3], private)
                if nc < 64:
                    assert np.any(cases[kind] != cut)


@pytest.mark.parametrize("nc", COLORS)
def test_one_wave_past_a_full_grid_stride(dev, nc):
    """BIG_N rows: every wave of the full grid runs one step, the first wave a
    second full one and the second wave a step of one row.  The rows are drawn
    from the six kinds of masks, so the statement counts a few hundred
    distinct masks."""
    small = cmp.mask_cases(257, nc, seed=nc)
    palette = np.concatenate([small[kind] for kind in KINDS])
    rng = np.random.default_rng(nc)
    masks = palette[rng.integers(0, len(palette), BIG_N)]
    masks[-1] = palette[3 * 257 + 5] | np.uint64(1 << (nc - 1))  # the lone last row holds the highest colour
    G, occ, private = _check(dev, masks, nc, twice=True)
    _identities(G, occ, private, BIG_N)
    assert int(G[nc - 1][nc - 1]) > 0


def test_alignment_null_outputs_and_refusals(dev):
    nc = 11
    masks = cmp.mask_cases(300, nc, seed=7)["dense"]
    want = cmp.as_arrays(*cmp.mask_gram(masks, nc))
    # d_masks at an address that is 8- but not 16-byte aligned
    _, G, o, p = _gram(dev, masks, nc, shift=8)
    for got, w in zip((G, o, p), want):
        np.testing.assert_array_equal(got, w)
    # NULL d_occ, NULL d_private: accepted, the others are filled
    for occ, private in ((False, True), (True, False), (False, False)):
        _, G, o, p = _gram(dev, masks, nc, occ=occ, private=private)
        np.testing.assert_array_equal(G, want[0])
        assert (o is None) == (not occ) and (p is None) == (not private)
        if occ:
            np.testing.assert_array_equal(o, want[1])
        if private:
            np.testing.assert_array_equal(p, want[2])
    # refused: every sentinel intact (checked in _gram)
    for bad in (0, 65):
        rc = _gram(dev, masks, bad, rc_want=N.KMAN_EINVAL)[0]
        assert rc == N.KMAN_EINVAL
    assert _gram(dev, masks, nc, gram=False, rc_want=N.KMAN_EINVAL)[0] == N.KMAN_EINVAL
    assert _gram(dev, masks, nc, n=N.KMAN_GRAM_MAX_ROWS + 1, rc_want=N.KMAN_EINVAL)[0] == N.KMAN_EINVAL
    # the context is still usable; n == 0 zeroes the outputs
    _, G, o, p = _gram(dev, masks[:0], nc)
    assert not G.any() and not o.any() and not p.any()
    _, G, o, p = _gram(dev, masks, nc)
    np.testing.assert_array_equal(G, want[0])


def test_launches_are_timed_under_gram(dev):
    from ctypes import byref, c_double, c_uint64

    L = N.lib()
    masks = cmp.mask_cases(100, 5, seed=1)["dense"]
    assert L.kman_timing_enable(dev.ctx, 1) == N.KMAN_OK
    try:
        _gram(dev, masks, 5)
        _gram(dev, masks[:0], 5)  # n == 0: no launch
        n, ms = c_uint64(0), c_double(0)
        assert L.kman_timing_query(dev.ctx, b"gram", byref(n), byref(ms)) == N.KMAN_OK
        assert n.value == 1 and ms.value > 0
    finally:
        L.kman_timing_enable(dev.ctx, 0)


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


@pytest.mark.parametrize("k", [5, 21, 32])
def test_engine_mask_gram_on_real_coloured_tables(dev, k):
    from kman_amd import engine

    inputs = cmp.planted_inputs(seed=k)
    for canonical in (False, True):
        want = cmp.as_arrays(*cmp.compare(inputs, k, canonical))
        tables = [_count_table(dev, r, k, canonical) for r in inputs]
        sizes = [int(t.n) for t in tables]
        ct = None
        try:
            ct = engine.color_table(dev, tables)
            G, occ, private = engine.mask_gram(dev, ct, len(inputs))
        finally:
            for t in tables:
                engine.free_result(t)
            engine.free_result(ct)
        for got, w in zip((G, occ, private), want):
            assert got.dtype == np.uint64 and got.shape == w.shape
            np.testing.assert_array_equal(got, w)
        assert [int(G[c][c]) for c in range(4)] == sizes  # each table's rows before folding
        assert sizes[3] == 0 and int(G[0][1]) > 0 and int(G[1][2]) > 0 and int(occ[3]) > 0
        # one pair against the set operation it replaces
        ta, tb = _count_table(dev, inputs[0], k, canonical), _count_table(dev, inputs[1], k, canonical)
        both = None
        try:
            both = engine.set_op(dev, ta, tb, "intersect")
            assert int(both.n) == int(G[0][1])
        finally:
            for t in (ta, tb, both):
                engine.free_result(t)
    # an empty coloured table gives zeros
    tables = [engine.empty_count(dev, k), engine.empty_count(dev, k)]
    ct = engine.color_table(dev, tables)
    try:
        G, occ, private = engine.mask_gram(dev, ct, 2)
    finally:
        engine.free_result(ct)
    assert G.shape == (2, 2) and occ.shape == (3,) and private.shape == (2,)
    assert not G.any() and not occ.any() and not private.any()


def test_engine_mask_gram_refuses(dev):
    from kman_amd import engine

    class _Narrow:
        k, n, count_bytes = 21, 0, 4

    with pytest.raises(AssertionError):
        engine.mask_gram(dev, _Narrow(), 2)
    _Narrow.count_bytes = 8
    for nc in (0, 65, True, 1.5):
        with pytest.raises(AssertionError):
            engine.mask_gram(dev, _Narrow(), nc)


# ------------------------------------------------------------------------ CLI


def _cli(*argv):
    from kman_amd.scripts.kmer import main

    r = CliRunner().invoke(main, [str(a) for a in argv], catch_exceptions=False)
    assert r.exit_code == 0, r.output


def _run(tmp, paths, inputs, k, argv=(), **kw):
    """`kmer compare` with every file, each byte for byte against the
    statement on `inputs` (the records the command should see)."""
    labels = [cc.label_of(str(p)) for p in paths]
    G, occ, private = cmp.compare(inputs, k, **kw)
    out, occf, summ = tmp / "out.tsv", tmp / "occ.tsv", tmp / "summary.tsv"
    _cli("compare", out, k, *paths, "--occupancy", occf, "--summary", summ, *argv)
    assert out.read_bytes() == cmp.lines(labels, G, k)
    assert out.read_bytes().count(b"\n") == len(paths) * (len(paths) - 1) // 2
    assert occf.read_bytes() == cmp.occupancy(occ)
    assert summ.read_bytes() == cmp.summary(labels, G, private)
    return labels, G, occ, private


def test_cli_end_to_end(tmp_path):
    import fastq_cases as fq
    from fastq_qual_cases import mask_fastq

    k = 9
    rng = np.random.default_rng(31)
    qtext = fq.mixed_reads(seed=8, n_records=60)
    reads = sc.fasta_records(fq.fastq_to_fasta(qtext))
    genome = [("g", "N".join(s for _, s in reads[:25]) + sc.rand_seq(rng, 200))]
    other = [("o%d" % i, s) for i, (_, s) in enumerate(reads[20:45])] + [("dup", reads[21][1])]
    paths = [tmp_path / "genome.fa", tmp_path / "other.fasta.gz", tmp_path / "reads.fq.gz", tmp_path / "copy.fa",
             tmp_path / "none.fa"]
    paths[0].write_bytes(sc.fasta(genome))
    with gzip.open(paths[1], "wb") as fh:
        fh.write(sc.fasta(other))
    with gzip.open(paths[2], "wb") as fh:
        fh.write(qtext)
    paths[3].write_bytes(sc.fasta(genome))  # the first input under another file name
    paths[4].write_bytes(b">short\nACGT\n")  # no k-mer: an empty table
    none = [("short", "ACGT")]
    inputs = [genome, other, reads, genome, none]
    labels, G, occ, private = _run(tmp_path, paths, inputs, k)
    assert labels == ["genome", "other", "reads", "copy", "none"]
    pair = [r for r in cmp.rows(G, k) if (r[0], r[1]) == (0, 3)][0]
    assert pair[5] == 1.0 and pair[8] == 0.0  # the duplicated input: J = 1, D = 0
    assert b"genome\tcopy\t%d\t%d\t%d\t1.000000\t1.000000\t1.000000\t0.000000\n" % (G[0][0], G[0][0], G[0][0]) \
        in (tmp_path / "out.tsv").read_bytes()
    assert G[0][1] > 0 and G[1][2] > 0 and G[4][4] == 0 and private[0] == 0 and occ[4] > 0
    _run(tmp_path, paths, inputs, k, ["--canonical"], canonical=True)
    _, G2, _, _ = _run(tmp_path, paths, inputs, k, ["-L", 2], min_count=2)
    assert 0 < G2[1][1] < G[1][1]
    _run(tmp_path, paths, inputs, k, ["--canonical", "-L", 2, "-U", 3], canonical=True, min_count=2, max_count=3)
    # -q masks the fastq input alone
    masked = sc.fasta_records(mask_fastq(qtext, 25, 33)[0])
    _, Gq, _, _ = _run(tmp_path, paths, [genome, other, masked, genome, none], k, ["-q", 25])
    assert Gq[2][2] < G[2][2] and Gq[0][0] == G[0][0]
    # --hpc: every input compressed before its k-mers are taken
    squeezed = [[(n, hc.hpc_seq(s)[0]) for n, s in recs] for recs in inputs]
    _, Gh, _, _ = _run(tmp_path, paths, squeezed, k, ["--hpc"])
    assert Gh != G
    # --matrix with each metric; dist is the default
    mat = tmp_path / "matrix.tsv"
    for metric in cmp.METRICS:
        _cli("compare", tmp_path / "out.tsv", k, *paths, "--matrix", mat, "--metric", metric)
        assert mat.read_bytes() == cmp.matrix(labels, G, k, metric), metric
        assert mat.read_bytes().startswith(b"5\ngenome\t")
    _cli("compare", tmp_path / "out.tsv", k, *paths, "--matrix", mat)
    assert mat.read_bytes() == cmp.matrix(labels, G, k, "dist")
    # two inputs, the fewest
    _run(tmp_path, paths[:2], inputs[:2], k)


def test_cli_sixty_four_inputs(tmp_path):
    k = 11
    rng = np.random.default_rng(5)
    base = sc.rand_seq(rng, 900)
    inputs, paths = [], []
    for i in range(64):
        recs = [("s%d" % i, base[11 * i:11 * i + 200]), ("p%d" % i, sc.rand_seq(rng, 30))]
        inputs.append(recs)
        paths.append(tmp_path / ("in%02d.fa" % i))
        paths[-1].write_bytes(sc.fasta(recs))
    labels, G, occ, private = _run(tmp_path, paths, inputs, k)
    assert G[63][63] > 0 and G[62][63] > 0 and G[0][63] == 0 and all(x > 0 for x in private)
    assert max(p for p in range(65) if occ[p]) > 10
