"""Two count tables on the GPU: kman_match_counts against the numpy statement
(tests/setop_cases.py), engine.set_op on the same tables, and `kmer sets`
pinned to set arithmetic on the reference's own `count` lines (tests/golden)
and, at k = 21 and 32, to np_oracle's counts of inputs that share records."""

from __future__ import annotations

import functools
import os
from ctypes import c_void_p

import numpy as np
import pytest

import setop_cases as sc
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

from kman_amd import _native as N  # noqa: E402

T = N.KMAN_MATCH_TILE
SMALL = [0, 1, T - 1, T, T + 1, 3 * T + 17]
BIG = (1 << 20) + 3
PAD = 64  # sentinel rows after `out`
DT = {4: np.uint32, 8: np.uint64}
SENT = {4: 0xA5A5A5A5, 8: 0xA5A5A5A5A5A5A5A5}


@pytest.fixture(scope="module")
def dev():
    from kman_amd import engine

    return engine.default_device()


class _Table:
    """Keys and counts on the device, from row `at` of their buffers (at = 1:
    no array starts on a 16-byte boundary)."""

    def __init__(self, dev, keys, counts, at=0):
        self.dev, self.n, self.cb, self.at = dev, len(keys), counts.dtype.itemsize, at
        self.hk = np.concatenate([np.zeros(at, np.uint64), np.asarray(keys, np.uint64)])
        self.hc = np.concatenate([np.zeros(at, counts.dtype), counts])
        self.k = dev.alloc(max(16, self.hk.nbytes))
        self.c = dev.alloc(max(16, self.hc.nbytes))
        if len(self.hk):
            dev.upload(self.k, self.hk)
            dev.upload(self.c, self.hc)

    @property
    def kp(self):
        return self.k.ptr + 8 * self.at

    @property
    def cp(self):
        return self.c.ptr + self.cb * self.at

    def unchanged(self):
        if len(self.hk):
            np.testing.assert_array_equal(self.dev.download(self.k, len(self.hk), np.uint64), self.hk)
            np.testing.assert_array_equal(self.dev.download(self.c, len(self.hc), self.hc.dtype), self.hc)

    def result(self, k=21):
        from kman_amd import engine

        return engine.CountResult(self.k, self.c, self.cb, self.n, k)

    def free(self):
        self.k.free()
        self.c.free()


def _match(dev, a: _Table, b: _Table, op: int, out, ob: int):
    return N.lib().kman_match_counts(dev.ctx, c_void_p(a.kp), c_void_p(a.cp), a.cb, a.n, c_void_p(b.kp),
                                     c_void_p(b.cp), b.cb, b.n, op, c_void_p(out.ptr), ob)


def _check_ops(dev, ak, ac, bk, bc, ob=4, ops=sc.MATCH_OPS, mixed=False, at=0):
    """Every op against the numpy statement; the PAD rows after out and both
    inputs are as they were."""
    assert np.all(ak[1:] > ak[:-1]) and np.all(bk[1:] > bk[:-1])  # (the precondition, on the test's own tables)
    hit, _ = sc.lookup(ak, bk, bc)
    if mixed:
        assert 0 < int(hit.sum()) < len(ak)  # (a test cannot pass by matching nothing, or everything)
    a, b = _Table(dev, ak, ac, at), _Table(dev, bk, bc, at)
    out = dev.alloc(ob * (len(ak) + PAD))
    fill = np.full(len(ak) + PAD, SENT[ob], DT[ob])
    try:
        for op in ops:
            dev.upload(out, fill)
            assert _match(dev, a, b, sc.MATCH_OPS.index(op), out, ob) == N.KMAN_OK, op
            got = dev.download(out, len(ak) + PAD, DT[ob])
            np.testing.assert_array_equal(got[:len(ak)], sc.match(ak, ac, bk, bc, op, ob), err_msg=op)
            np.testing.assert_array_equal(got[len(ak):], fill[len(ak):], err_msg=op)
        a.unchanged()
        b.unchanged()
    finally:
        for x in (a, b, out):
            x.free()
    return int(hit.sum())


# ------------------------------------------------------------ kernel vs numpy


@pytest.mark.parametrize("nb", SMALL)
@pytest.mark.parametrize("na", SMALL)
def test_match_all_pairs_of_small_sizes(dev, na, nb):
    rng = np.random.default_rng(na * 7919 + nb)
    for pattern in sc.GENERAL:
        ak, bk = sc.tables(pattern, na, nb)
        _check_ops(dev, ak, sc.counts_for(rng, na, 4), bk, sc.counts_for(rng, nb, 4),
                   mixed=pattern in sc.MIXED and min(na, nb) >= T - 1)


@pytest.mark.parametrize("na, nb", [(BIG, T + 1), (T + 1, BIG), (BIG, BIG)])
def test_match_large(dev, na, nb):
    rng = np.random.default_rng(na + 3 * nb)
    for pattern in ("random", "extremes_both", "interleaved"):
        ak, bk = sc.tables(pattern, na, nb)
        _check_ops(dev, ak, sc.counts_for(rng, na, 4), bk, sc.counts_for(rng, nb, 4), mixed=pattern in sc.MIXED,
                   ops=("right", "sum", "absent", "any_max"))


@pytest.mark.parametrize("n", [1, T - 1, T, T + 1, 3 * T + 17, BIG])
def test_identical_and_shifted_by_one_row(dev, n):
    """B = A: every row matched.  B = one smaller key, then A: every equal
    pair moved across the tile boundaries (the row past a tile's B slice)."""
    rng = np.random.default_rng(n)
    ops = sc.MATCH_OPS if n < BIG else ("right", "min", "absent")
    for ak, bk in (sc.identical(n), sc.shifted(n)):
        hits = _check_ops(dev, ak, sc.counts_for(rng, len(ak), 4), bk, sc.counts_for(rng, len(bk), 4), ops=ops)
        assert hits == n
    bk, ak = sc.shifted(n)  # the roles swapped: A's first row alone is unmatched
    hits = _check_ops(dev, ak, sc.counts_for(rng, len(ak), 4), bk, sc.counts_for(rng, len(bk), 4), ops=ops, mixed=True)
    assert hits == n


@pytest.mark.parametrize("ends", [False, True])
def test_many_rows_packed_between_two_neighbouring_keys(dev, ends):
    rng = np.random.default_rng(5 + ends)
    ak, bk = sc.packed(5, 3 * T, ends)
    assert _check_ops(dev, ak, sc.counts_for(rng, 5, 4), bk, sc.counts_for(rng, 3 * T, 4), mixed=ends) == 2 * ends
    # the roles swapped: 3 T rows of A between two neighbouring keys of a 5-row B
    assert _check_ops(dev, bk, sc.counts_for(rng, 3 * T, 4), ak, sc.counts_for(rng, 5, 4), mixed=ends) == 2 * ends


def test_extreme_keys(dev):
    """Keys 0 and 2^64 - 1 in both tables and in one only: no value is a sentinel."""
    rng = np.random.default_rng(3)
    lo, hi = 0, sc.U64_MAX
    mid = [5, 1 << 40, (1 << 63) + 9]
    for a_ext, b_ext in (((lo, hi), (lo, hi)), ((lo, hi), ()), ((), (lo, hi)), ((lo,), (hi,)), ((hi,), (hi,))):
        ak = np.asarray(sorted(set(mid) | set(a_ext)), np.uint64)
        bk = np.asarray(sorted(set(mid[:2]) | set(b_ext)), np.uint64)
        hits = _check_ops(dev, ak, sc.counts_for(rng, len(ak), 4), bk, sc.counts_for(rng, len(bk), 4), mixed=True)
        assert hits == 2 + len(set(a_ext) & set(b_ext))
    ak, bk = np.asarray([lo, hi], np.uint64), np.asarray([lo, hi], np.uint64)
    assert _check_ops(dev, ak, sc.counts_for(rng, 2, 4), bk, sc.counts_for(rng, 2, 4)) == 2
    assert _check_ops(dev, ak, sc.counts_for(rng, 2, 4), np.asarray([7], np.uint64), sc.counts_for(rng, 1, 4)) == 0


@pytest.mark.parametrize("ob", [4, 8])
@pytest.mark.parametrize("ab, bb", [(4, 4), (4, 8), (8, 4), (8, 8)])
def test_count_widths(dev, ab, bb, ob):
    """u64 counts are above 2^32: they saturate a 4-byte out."""
    rng = np.random.default_rng(ab * 100 + bb * 10 + ob)
    for na, nb in ((3 * T + 17, T + 1), (T + 1, 3 * T + 17)):
        ak, bk = sc.tables("random", na, nb, seed=ab + bb)
        ac, bc = sc.counts_for(rng, na, ab), sc.counts_for(rng, nb, bb)
        _check_ops(dev, ak, ac, bk, bc, ob, mixed=True)
        if ob == 4 and 8 in (ab, bb):
            assert int((sc.match(ak, ac, bk, bc, "sum", 4) == sc.U32_MAX).sum()) > 0


@pytest.mark.parametrize("ob", [4, 8])
def test_sum_saturates(dev, ob):
    n = T + 1
    ak, bk = sc.identical(n)
    top = sc.U32_MAX if ob == 4 else sc.U64_MAX
    dt = DT[ob]
    # ca + cb: one below the largest value, equal to it, one above it, far above it
    ac = np.tile(np.asarray([top - 6, top - 5, top - 4, top - 1], dt), n // 4 + 1)[:n]
    bc = np.full(n, 5, dt)
    for op in ("sum", "any_sum"):
        want = sc.match(ak, ac, bk, bc, op, ob)
        assert sorted(set(want.tolist())) == [top - 1, top]
    _check_ops(dev, ak, ac, bk, bc, ob)
    if ob == 4:  # the same counts into a u64 out: exact
        assert int(sc.match(ak, ac, bk, bc, "sum", 8).max()) == top + 4
        _check_ops(dev, ak, ac, bk, bc, 8, ops=("sum", "any_sum", "max"))


def test_arrays_that_are_not_16_byte_aligned(dev):
    rng = np.random.default_rng(11)
    for ab, bb in ((4, 4), (8, 8), (4, 8)):
        for na, nb in ((3 * T + 18, T + 2), (T, 3 * T + 17)):
            ak, bk = sc.tables("random", na, nb, seed=9)
            _check_ops(dev, ak, sc.counts_for(rng, na, ab), bk, sc.counts_for(rng, nb, bb), 4, mixed=True, at=1)


def test_refused_calls(dev):
    rng = np.random.default_rng(1)
    n = T + 1
    ak, bk = sc.tables("random", n, n)
    ac, bc = sc.counts_for(rng, n, 4), sc.counts_for(rng, n, 4)
    a, b = _Table(dev, ak, ac), _Table(dev, bk, bc)
    out = dev.alloc(4 * (n + PAD))
    fill = np.full(n + PAD, SENT[4], np.uint32)
    dev.upload(out, fill)
    L = N.lib()
    try:
        for op in (-1, 8, 100):
            assert _match(dev, a, b, op, out, 4) == N.KMAN_EINVAL
        for widths in ((2, 4, 4), (4, 0, 4), (4, 4, 16), (4, 4, 2), (16, 4, 4), (4, 12, 8)):
            rc = L.kman_match_counts(dev.ctx, c_void_p(a.kp), c_void_p(a.cp), widths[0], n, c_void_p(b.kp),
                                     c_void_p(b.cp), widths[1], n, N.KMAN_MATCH_SUM, c_void_p(out.ptr), widths[2])
            assert rc == N.KMAN_EINVAL, widths
        np.testing.assert_array_equal(dev.download(out, n + PAD, np.uint32), fill)  # nothing was written
        # na == 0: nothing is launched; nb == 0 with no B at all: every row unmatched
        assert L.kman_match_counts(dev.ctx, None, None, 4, 0, c_void_p(b.kp), c_void_p(b.cp), 4, n,
                                   N.KMAN_MATCH_SUM, None, 4) == N.KMAN_OK
        assert L.kman_match_counts(dev.ctx, c_void_p(a.kp), c_void_p(a.cp), 4, n, None, None, 4, 0,
                                   N.KMAN_MATCH_ANY_SUM, c_void_p(out.ptr), 4) == N.KMAN_OK
        got = dev.download(out, n + PAD, np.uint32)
        np.testing.assert_array_equal(got[:n], ac)
        np.testing.assert_array_equal(got[n:], fill[n:])
        # the context is still usable
        assert _match(dev, a, b, N.KMAN_MATCH_RIGHT, out, 4) == N.KMAN_OK
        np.testing.assert_array_equal(dev.download(out, n, np.uint32), sc.match(ak, ac, bk, bc, "right"))
    finally:
        for x in (a, b, out):
            x.free()


# ----------------------------------------------------------------- engine API


def _engine_cases():
    return [(op, c) for op, cs in sc.SET_COUNTS.items() for c in cs + (None,)]


@pytest.mark.parametrize("ab, bb", [(4, 4), (4, 8)])
@pytest.mark.parametrize("na, nb", [(3 * T + 17, T + 1), (T + 1, 3 * T + 17), (T, 0), (0, T)])
def test_engine_set_op(dev, na, nb, ab, bb):
    from kman_amd import engine

    rng = np.random.default_rng(na + 5 * nb + ab + bb)
    ak, bk = sc.tables("random", na, nb, seed=4)
    ac, bc = sc.counts_for(rng, na, ab, small=True), sc.counts_for(rng, nb, bb, small=True)
    ob = 8 if 8 in (ab, bb) else 4
    off = (1 << 32) if bb == 8 else 0  # (u64 counts sit above 2^32: ranges that split them)
    a, b = _Table(dev, ak, ac), _Table(dev, bk, bc)
    try:
        ra, rb = a.result(), b.result()
        v = engine.match_counts(dev, ra, rb)
        try:
            assert v.nbytes >= ob * max(na, 1)
            np.testing.assert_array_equal(dev.download(v, na, DT[ob]), sc.match(ak, ac, bk, bc, "right", ob))
        finally:
            v.free()
        for op, counts in _engine_cases():
            for lo, hi in ((1, None), (2, None), (off + 2, off + 7), (3, 3)):
                wk, wc = sc.set_op(ak, ac, bk, bc, op, counts, lo, hi, ob)
                if min(na, nb) and (lo, hi) == (1, None):
                    assert 0 < len(wk) < na + nb
                r = engine.set_op(dev, ra, rb, op, counts, lo, hi)
                try:
                    assert (r.n, r.k, r.count_bytes) == (len(wk), 21, ob)
                    assert r.ukeys is not a.k and r.ukeys is not b.k
                    gk, gc = engine.download_count(dev, r)
                    np.testing.assert_array_equal(gk, wk, err_msg=str((op, counts, lo, hi)))
                    np.testing.assert_array_equal(gc, wc, err_msg=str((op, counts, lo, hi)))
                    assert np.all(gk[1:] > gk[:-1])  # strictly ascending (union: the merge of two disjoint runs)
                finally:
                    engine.free_result(r)
        assert (ra.n, rb.n) == (na, nb)
        a.unchanged()
        b.unchanged()
    finally:
        a.free()
        b.free()


# ------------------------------------------------------------------------ CLI


def _cli(*argv):
    from kman_amd.scripts.kmer import main

    main([str(a) for a in argv], standalone_mode=False)


def _ref(name: str) -> bytes:
    with open(os.path.join(GOLDEN, "ref_outputs", name + ".txt"), "rb") as fh:
        return fh.read()


# (k, A, B, rows of A alone / shared / of B alone on the reference's forward lines)
GOLDEN_PAIRS = [(5, "messy1", "edge", 994, 24, 0), (5, "messy2", "messy1", 6, 1018, 0), (3, "messy1", "edge", 48, 16, 0)]


@pytest.mark.parametrize("variant", ["plain", "reverse", "min_count_2"])
@pytest.mark.parametrize("op", ["intersect", "subtract", "union"])
@pytest.mark.parametrize("k, a, b, only_a, shared, only_b", GOLDEN_PAIRS)
def test_sets_pinned_to_reference_lines(golden_inputs, tmp_path, k, a, b, only_a, shared, only_b, op, variant):
    sfx = "__r" if variant == "reverse" else ""
    a_text, b_text = _ref("%s__count__k%d%s" % (a, k, sfx)), _ref("%s__count__k%d%s" % (b, k, sfx))
    lo = 2 if variant == "min_count_2" else 1
    want = sc.lines_set_op(a_text, b_text, op, None, lo)
    if variant == "plain":  # the pair is mixed
        assert len(want.splitlines()) == {"intersect": shared, "subtract": only_a, "union": only_a + shared + only_b}[op]
        assert only_a > 0 and shared > 0
    flags = {"plain": [], "reverse": ["-r"], "min_count_2": ["-L", 2]}[variant]
    out = tmp_path / "got.txt"
    _cli("sets", golden_inputs[a], golden_inputs[b], out, k, "--op", op, *flags)
    assert out.read_bytes() == want


@pytest.mark.parametrize("op, counts", [("intersect", "right"), ("intersect", "min"), ("intersect", "max"),
                                        ("intersect", "sum"), ("intersect", "left"), ("subtract", "left"),
                                        ("union", "max"), ("union", "sum")])
def test_sets_counts_choices_on_reference_lines(golden_inputs, tmp_path, op, counts):
    a_text, b_text = _ref("messy1__count__k5"), _ref("edge__count__k5")
    want = sc.lines_set_op(a_text, b_text, op, counts, 3, 8)
    assert 0 < len(want.splitlines()) < len(sc.lines_set_op(a_text, b_text, op, counts).splitlines())
    out = tmp_path / "got.txt"
    _cli("sets", golden_inputs["messy1"], golden_inputs["edge"], out, 5, "--op", op, "--counts", counts,
         "--min-count", 3, "--max-count", 8)
    assert out.read_bytes() == want
    # gzipped INPUT_A
    _cli("sets", golden_inputs["messy1.gz"], golden_inputs["edge"], out, 5, "--op", op, "--counts", counts, "-L", 3,
         "-U", 8)
    assert out.read_bytes() == want


def _fasta(records) -> bytes:
    return b"".join(b">" + t + b"\n" + s + b"\n" for t, s in records)


@functools.lru_cache(maxsize=None)
def _shared_pair():
    """A: messy records; B: every second record of A plus records of its own."""
    import inputs
    import np_oracle

    a_text = inputs.messy_records(11, n_records=12, max_len=4000)
    a_recs = np_oracle.parse_fasta(a_text)
    own = np_oracle.parse_fasta(inputs.messy_records(12, n_records=8, max_len=4000))
    return a_text, _fasta(a_recs[::2] + [(b"own_" + t, s) for t, s in own])


@functools.lru_cache(maxsize=None)
def _np_rows(text: bytes, k: int, rc: bool = False, canonical: bool = False):
    import np_oracle

    keys, _ = np_oracle.stream_kmers(np_oracle.parse_fasta(text), k, rc=rc, canonical=canonical)
    return np_oracle.rle_count(np.sort(keys))


@pytest.mark.parametrize("mode", ["forward", "canonical", "reverse"])
@pytest.mark.parametrize("k", [21, 32])
def test_sets_matches_np_oracle_on_shared_records(tmp_path, k, mode):
    a_text, b_text = _shared_pair()
    (tmp_path / "a.fa").write_bytes(a_text)
    (tmp_path / "b.fa").write_bytes(b_text)
    ak, ac = _np_rows(a_text, k, mode == "reverse", mode == "canonical")
    bk, bc = _np_rows(b_text, k, mode == "reverse", mode == "canonical")
    hit, _ = sc.lookup(ak, bk, bc)
    assert 0 < int(hit.sum()) < min(len(ak), len(bk))  # shared k-mers, and k-mers of each input alone
    flags = {"forward": [], "canonical": ["--canonical"], "reverse": ["-r"]}[mode]
    out = tmp_path / "got.txt"
    for op, counts, lo in (("intersect", None, 1), ("intersect", "sum", 1), ("subtract", None, 1), ("union", None, 1),
                           ("union", "sum", 2), ("union", "max", 1)):
        wk, wc = sc.set_op(ak, ac, bk, bc, op, counts, lo)
        assert len(wk)
        _cli("sets", tmp_path / "a.fa", tmp_path / "b.fa", out, k, "--op", op, *flags,
             *(["--counts", counts] if counts else []), *(["-L", lo] if lo > 1 else []))
        assert out.read_bytes() == sc.rows_to_lines(wk, wc, k), (op, counts, lo)


def test_sets_fastq_against_fasta_with_min_qual(tmp_path):
    """-q masks the fastq input only; the fasta input holds half of its reads unmasked."""
    import fastq_cases as fq
    import np_oracle
    from fastq_qual_cases import mask_fastq

    k = 11
    reads = fq.short_reads(60_000)
    masked, n_masked = mask_fastq(reads, 20, 33)
    assert n_masked > 0
    recs = np_oracle.parse_fasta(fq.fastq_to_fasta(reads))
    own = np_oracle.parse_fasta(fq.fastq_to_fasta(fq.short_reads(20_000, seed=8)))
    b_text = _fasta(recs[::2] + own)
    (tmp_path / "reads.fq").write_bytes(reads)
    (tmp_path / "b.fa").write_bytes(b_text)
    ak, ac = _np_rows(masked, k)
    bk, bc = _np_rows(b_text, k)
    unmasked_k, _ = _np_rows(fq.fastq_to_fasta(reads), k)
    assert len(ak) < len(unmasked_k)  # (the mask removed k-mers)
    out = tmp_path / "got.txt"
    for op, x, y in (("intersect", "reads.fq", "b.fa"), ("subtract", "reads.fq", "b.fa"),
                     ("subtract", "b.fa", "reads.fq"), ("union", "b.fa", "reads.fq")):
        first = (ak, ac, bk, bc) if x == "reads.fq" else (bk, bc, ak, ac)
        wk, wc = sc.set_op(*first, op)
        assert 0 < len(wk) < len(ak) + len(bk)
        _cli("sets", tmp_path / x, tmp_path / y, out, k, "--op", op, "-q", 20)
        assert out.read_bytes() == sc.rows_to_lines(wk, wc, k), (op, x)


def test_sets_input_without_kmers_is_the_empty_set(tmp_path):
    a_text, _ = _shared_pair()
    (tmp_path / "a.fa").write_bytes(a_text)
    (tmp_path / "none.fa").write_bytes(b">x\nACGTACG\n>y\nNNNN\n")
    ak, ac = _np_rows(a_text, 21)
    whole = sc.rows_to_lines(ak, ac, 21)
    out = tmp_path / "got.txt"
    for x, y, op, want in (("a.fa", "none.fa", "intersect", b""), ("a.fa", "none.fa", "subtract", whole),
                           ("a.fa", "none.fa", "union", whole), ("none.fa", "a.fa", "union", whole),
                           ("none.fa", "a.fa", "subtract", b""), ("none.fa", "none.fa", "union", b"")):
        _cli("sets", tmp_path / x, tmp_path / y, out, 21, "--op", op)
        assert out.read_bytes() == want, (x, y, op)


def test_sets_refusals_and_input_errors(golden_inputs, tmp_path):
    out = tmp_path / "got.txt"
    with pytest.raises(AssertionError, match="K <= 32"):
        _cli("sets", golden_inputs["messy1"], golden_inputs["edge"], out, 33, "--op", "union")
    for bad in ("empty", "noheader"):  # as `count` raises for them
        with pytest.raises(AssertionError):
            _cli("count", golden_inputs[bad], tmp_path / "c.txt", 5)
        for x, y in ((bad, "edge"), ("edge", bad)):
            with pytest.raises(AssertionError):
                _cli("sets", golden_inputs[x], golden_inputs[y], out, 5, "--op", "union")
    assert not out.exists()
