"""Isolated substitution errors repaired on the GPU: kman_correct_sites and
kman_apply_fixes on hand-built inputs, engine.correct and `kmer screen --solid
C --correct`, all for exact equality with the plain-Python statement
(tests/correct_cases.py)."""

from __future__ import annotations

import gzip
from ctypes import byref, c_uint64, c_void_p

import numpy as np
import pytest
from click.testing import CliRunner

import correct_cases as cc
import median_cases as mc
import reads_cases as rc
import screen_cases as sc
import solid_cases as so

pytestmark = pytest.mark.gpu

from kman_amd import _native as N  # noqa: E402

T = N.KMAN_CORRECT_TILE
CAP = N.KMAN_CORRECT_REC_CAP
NOFIX = N.KMAN_FIX_NONE
PAD = 64       # sentinel bytes after an output
SENT = 0xA5


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


class _Table:
    """A k-mer -> count dict on the device: key-sorted rows and their prefix index."""

    def __init__(self, dev, table, k, count_bytes=4, index_bits=None):
        from kman_amd import engine

        self.keys, self.counts = sc.table_rows(table, count_bytes)
        self.k, self.nt, self.count_bytes = k, len(self.keys), count_bytes
        self.bits = engine.default_index_bits(self.nt, k) if index_bits is None else index_bits
        self.bufs = [_up(dev, self.keys), _up(dev, self.counts), dev.alloc(8 * ((1 << self.bits) + 1))]
        N.check(dev.ctx, N.lib().kman_table_index(dev.ctx, c_void_p(self.bufs[0].ptr), self.nt, k, self.bits,
                                                  c_void_p(self.bufs[2].ptr)), "kman_table_index")

    def free(self):
        for b in self.bufs:
            b.free()


def _sites(dev, codes, words, rec_seq, n, t, C, canonical=False, null=None, n_records=None, **over):
    """One kman_correct_sites call: (return code, d_fix with the sentinel bytes
    after it, *n_fixed).  The codes and words must come back unchanged."""
    codes = np.ascontiguousarray(codes, dtype=np.uint8)
    words = np.ascontiguousarray(words, dtype=np.uint32)
    rec_seq = np.ascontiguousarray(rec_seq, dtype=np.uint64)
    bufs = [_up(dev, codes), _up(dev, words), _up(dev, rec_seq), _up(dev, np.full(n + PAD, SENT, np.uint8))]
    try:
        ptrs = [b.ptr for b in bufs] + [t.bufs[0].ptr, t.bufs[1].ptr, t.bufs[2].ptr]
        if null is not None:
            ptrs[null] = None
        got = c_uint64(12345)
        a = dict(k=t.k, flags=N.KMAN_CANONICAL if canonical else 0, count_bytes=t.count_bytes, bits=t.bits, C=C)
        a.update(over)
        rc_ = N.lib().kman_correct_sites(
            dev.ctx, c_void_p(ptrs[0]), n, a["k"], a["flags"], c_void_p(ptrs[1]), c_void_p(ptrs[2]),
            len(rec_seq) if n_records is None else n_records, c_void_p(ptrs[4]), c_void_p(ptrs[5]), a["count_bytes"],
            t.nt, c_void_p(ptrs[6]), a["bits"], a["C"], c_void_p(ptrs[3]), byref(got))
        raw = dev.download(bufs[3], n + PAD, np.uint8)
        np.testing.assert_array_equal(dev.download(bufs[0], len(codes), np.uint8), codes)
        if len(words):
            np.testing.assert_array_equal(dev.download(bufs[1], len(words), np.uint32), words)
        return rc_, raw, got.value
    finally:
        for b in bufs:
            b.free()


def _check(dev, records, k, table, C, canonical=False, count_bytes=4, index_bits=None):
    """kman_correct_sites on the records' codes and the statement's words
    against the statement's plane; the plane."""
    codes, rec_seq, n = sc.codes_of(records)
    words = mc.window_words(records, k, table, canonical)
    want = cc.fix_plane(codes[:n].tolist(), words, rec_seq, n, k, table, C, canonical)
    t = _Table(dev, table, k, count_bytes, index_bits)
    try:
        rc_, raw, nf = _sites(dev, codes, words, rec_seq, n, t, C, canonical)
        assert rc_ == N.KMAN_OK, N.lib().kman_last_error(dev.ctx)
        assert raw[:n].tolist() == want
        assert np.all(raw[n:] == SENT)  # bytes past the plane untouched
        assert nf == sum(1 for f in want if f != NOFIX)
        rc2, raw2, nf2 = _sites(dev, codes, words, rec_seq, n, t, C, canonical)
        assert rc2 == N.KMAN_OK and raw2.tobytes() == raw.tobytes() and nf2 == nf  # two calls: identical bytes
    finally:
        t.free()
    return want


# ------------------------------------------------------------ the hand cases


@pytest.mark.parametrize("count_bytes", [4, 8])
@pytest.mark.parametrize("canonical", [False, True])
@pytest.mark.parametrize("k", [4, 21, 31, 32])
def test_hand_cases(dev, k, canonical, count_bytes):
    for name, recs, table, C, expected in cc.hand_cases(k, canonical):
        n = sum(len(s) for _, s in recs)
        assert _check(dev, recs, k, table, C, canonical, count_bytes) == cc.expected_plane(n, expected), name


def test_hand_cases_in_one_input(dev):
    """The hand cases that share the genome's table as the records of one input, and a narrow index."""
    k = 21
    every = cc.hand_cases(k)
    cases = [c for c in every if c[2] == every[0][2]]
    recs = [("%s_%s" % (c[0], nm), s) for c in cases for nm, s in c[1]]
    assert len(recs) > 12
    want = _check(dev, recs, k, cases[0][2], 3, index_bits=3)
    assert sum(1 for f in want if f != NOFIX) == sum(len(c[4]) for c in cases)


# --------------------------------------------------------------- edge shapes


def _genome(n, seed):
    return sc.rand_seq(np.random.default_rng(seed), n)


@pytest.mark.parametrize("canonical", [False, True])
def test_runs_at_tile_borders(dev, canonical):
    k, C = 21, 3
    g = _genome(T + 300, 1)
    table = cc.kmer_table([g], k, canonical)
    code = "ACGT".index
    # the run starts in the last k bases of tile 0 and ends in tile 1
    for p in (T + 5, T - 1, T, T + k - 2, T - k, T + k - 1):
        want = _check(dev, [("r", cc.sub(g, p))], k, table, C, canonical)
        assert want == cc.expected_plane(len(g), {p: code(g[p])}), p
    # a site at the very last window of the input, one at the first base; a second record that ends at a tile border
    recs = [("a", cc.sub(g[:T - 100], 0)), ("b", g[T - 100:T][:100]), ("c", cc.sub(g[:400], 399, 2))]
    want = _check(dev, recs, k, table, C, canonical)
    assert want == cc.expected_plane(T + 400, {0: code(g[0]), T + 399: code(g[399])})


def test_more_records_in_a_tile_than_the_lds_slice(dev):
    k, C = 15, 3
    g = _genome(200, 2)
    table = cc.kmer_table([g], k)
    tiny = [("t%d" % i, "A" if i % 2 == 0 else "") for i in range(2 * (CAP + 5))]
    recs = [("a", cc.sub(g[:150], 70))] + tiny + [("b", cc.sub(g[20:170], 0)), ("c", cc.sub(g[50:], 149, 3))]
    _, rec_seq, n = sc.codes_of(recs)
    assert n < T and len(rec_seq) > CAP  # every record in tile 0: the slice is searched in global memory
    want = _check(dev, recs, k, table, C)
    assert sum(1 for f in want if f != NOFIX) == 3
    # the same after a first tile that is one record: > CAP entries in tile 1
    lead = _genome(T - 10, 3)
    want = _check(dev, [("lead", lead)] + recs, k, cc.kmer_table([g, lead], k), C)
    assert sum(1 for f in want if f != NOFIX) == 3


def _tile_of_tiny_records(entries):
    """Tile 0 holds exactly T bases and `entries` records: three reads, then
    one-base and empty records up to its last base; tile 1 is one read."""
    g, lead = _genome(200, 2), _genome(T, 3)
    tiny = ["", "A"] * ((entries - 3) // 2)
    tiny = ["A"] * ((entries - 3) % 2) + tiny  # (ends with a one-base record: no empty one slips to base T)
    fill = T - 300 - tiny.count("A")
    recs = [("a", cc.sub(g[:150], 70)), ("lead", lead[:fill]), ("b", cc.sub(g[20:170], 0))]
    recs += [("t%d" % i, s) for i, s in enumerate(tiny)] + [("c", cc.sub(g[50:], 149, 3))]
    return recs, cc.kmer_table([g, lead], 15)


@pytest.mark.parametrize("entries", [CAP, CAP + 1])
def test_a_tile_with_exactly_the_lds_slice_and_one_more(dev, entries):
    """The fullest tile's slice of d_rec_seq has exactly CAP entries (the
    largest that is staged in LDS) and CAP + 1 (the smallest searched in
    global memory)."""
    recs, table = _tile_of_tiny_records(entries)
    _, rec_seq, n = sc.codes_of(recs)
    per_tile = np.bincount((rec_seq // T).astype(np.int64))
    assert n == T + 150 and per_tile.tolist() == [entries, 1] and rec_seq[0] == 0 and rec_seq[-1] == T
    want = _check(dev, recs, 15, table, 3)
    assert sum(1 for f in want if f != NOFIX) == 3


def test_one_long_record(dev):
    k, C = 21, 3
    g = _genome(10_000, 4)
    table = cc.kmer_table([g], k)
    at = [0, T - 3, 2 * T + 2, 5000, 9_999]  # both ends, runs across the borders at T and 2 T
    read = g
    for p in at:
        read = cc.sub(read, p)
    want = _check(dev, [("long", read)], k, table, C)
    assert want == cc.expected_plane(len(g), {p: "ACGT".index(g[p]) for p in at})


def test_tiny_and_empty_inputs(dev):
    k = 8
    g = _genome(60, 5)
    table = cc.kmer_table([g], k)
    t = _Table(dev, table, k)
    try:
        # n_bases < k: the plane is filled, nothing is corrected
        codes, rec_seq, n = sc.codes_of([("a", "ACG"), ("b", "TT")])
        rc_, raw, nf = _sites(dev, codes, [mc.NONE] * n, rec_seq, n, t, 3)
        assert rc_ == N.KMAN_OK and np.all(raw[:n] == NOFIX) and np.all(raw[n:] == SENT) and nf == 0
        # n_records == 0: the same
        read = cc.sub(g, 30)
        codes, rec_seq, n = sc.codes_of([("r", read)])
        words = mc.window_words([("r", read)], k, table)
        rc_, raw, nf = _sites(dev, codes, words, rec_seq, n, t, 3, n_records=0)
        assert rc_ == N.KMAN_OK and np.all(raw[:n] == NOFIX) and np.all(raw[n:] == SENT) and nf == 0
        rc_, raw, nf = _sites(dev, codes, words, rec_seq, n, t, 3)
        assert rc_ == N.KMAN_OK and nf == 1 and raw[30] == "ACGT".index(g[30])
        # n_bases == 0: nothing is done
        rc_, raw, nf = _sites(dev, codes[:0].tolist() + [4] * 64, [], [0], 0, t, 3)
        assert rc_ == N.KMAN_OK and np.all(raw == SENT) and nf == 0
        # an empty table: no window is solid, nothing is named
        e = _Table(dev, {}, k)
        try:
            rc_, raw, nf = _sites(dev, codes, [0 if w != mc.NONE else w for w in words], rec_seq, n, e, 1)
            assert rc_ == N.KMAN_OK and np.all(raw[:n] == NOFIX) and nf == 0
        finally:
            e.free()
    finally:
        t.free()


def test_refusals_write_nothing(dev):
    k = 8
    g = _genome(80, 6)
    table = cc.kmer_table([g], k)
    read = cc.sub(g, 40)
    codes, rec_seq, n = sc.codes_of([("r", read)])
    words = mc.window_words([("r", read)], k, table)
    t = _Table(dev, table, k)
    try:
        for kw in (dict(C=0), dict(C=0xFFFFFFFF), dict(bits=0), dict(bits=2 * k + 1), dict(bits=25), dict(k=1),
                   dict(k=33), dict(flags=1), dict(flags=N.KMAN_CANONICAL | 8), dict(count_bytes=2), dict(null=0),
                   dict(null=1), dict(null=2), dict(null=3), dict(null=4), dict(null=5), dict(null=6)):
            rc_, raw, nf = _sites(dev, codes, words, rec_seq, n, t, kw.pop("C", 3), **kw)
            assert rc_ == N.KMAN_EINVAL, kw
            assert np.all(raw == SENT) and nf == 0, kw  # the plane untouched
        rc_, raw, nf = _sites(dev, codes, words, rec_seq, n, t, 3)  # the context is still usable
        assert rc_ == N.KMAN_OK and nf == 1 and raw[40] == "ACGT".index(g[40])
    finally:
        t.free()


# ------------------------------------------------------------ the random case


@pytest.fixture(scope="module")
def random_case():
    k, C = 15, 3
    genome, reads, clean = cc.random_case()
    assert len(genome) == 2000 and len(reads) == 200 and all(len(s) == 100 for _, s in reads)
    table = cc.kmer_table([genome], k)
    assert set(table.values()) == {5}
    fix = cc.fix_plane_of(reads, k, table, C)
    fixed = cc.corrected(reads, fix)
    _, rec_seq, n = sc.codes_of(reads)
    sites = cc.named_sites(mc.window_words(reads, k, table), rec_seq, n, k, C)
    assert any(r != c and f == c for r, c, f in zip(reads, clean, fixed))  # a read fully repaired
    assert any(fix[p] == NOFIX for p in sites)                               # a site left alone
    return k, C, reads, table, fix


@pytest.mark.parametrize("canonical", [False, True])
def test_random_reads(dev, random_case, canonical):
    k, C, reads, table, fix = random_case
    if canonical:
        table = {min(w, sc.revcomp(w)): c for w, c in table.items()}
        assert _check(dev, reads, k, table, C, True) == cc.fix_plane_of(reads, k, table, C, True)
    else:
        assert _check(dev, reads, k, table, C) == fix


# ------------------------------------------------------------ kman_apply_fixes


def _apply(dev, codes, fix, rec_seq, n, text=None, off=None, null=None):
    """One kman_apply_fixes call: (return code, codes, nfix, text), each with
    its sentinel bytes; d_fix must come back unchanged."""
    codes = np.ascontiguousarray(codes, dtype=np.uint8)
    fix = np.ascontiguousarray(fix, dtype=np.uint8)
    rec_seq = np.ascontiguousarray(rec_seq, dtype=np.uint64)
    R = len(rec_seq)
    tb = np.concatenate([np.frombuffer(text, np.uint8), np.full(PAD, SENT, np.uint8)]) if text is not None else None
    bufs = [_up(dev, codes), _up(dev, fix), _up(dev, rec_seq), _up(dev, np.full(R + 16, 0xA5A5A5A5, np.uint32))]
    if text is not None:
        bufs += [_up(dev, tb), _up(dev, np.asarray(off, dtype=np.uint64))]
    try:
        ptrs = [b.ptr for b in bufs] + [None, None]
        if null is not None:
            ptrs[null] = None
        rc_ = N.lib().kman_apply_fixes(dev.ctx, c_void_p(ptrs[0]), n, c_void_p(ptrs[1]), c_void_p(ptrs[2]), R,
                                       c_void_p(ptrs[4]) if ptrs[4] else None, len(text) if text is not None else 0,
                                       c_void_p(ptrs[5]) if ptrs[5] else None, c_void_p(ptrs[3]))
        np.testing.assert_array_equal(dev.download(bufs[1], len(fix), np.uint8), fix)
        out_text = dev.download(bufs[4], len(tb), np.uint8).tobytes() if text is not None else None
        return rc_, dev.download(bufs[0], len(codes), np.uint8), dev.download(bufs[3], R + 16, np.uint32), out_text
    finally:
        for b in bufs:
            b.free()


def _fastq(records, nl=b"\n", quals=None):
    out = []
    for i, (name, seq) in enumerate(records):
        q = quals[i] if quals else "I" * len(seq)
        out.append(b"@" + name.encode() + b" d" + nl + seq.encode() + nl + b"+" + nl + q.encode() + nl)
    return b"".join(out)


@pytest.mark.parametrize("nl", [b"\n", b"\r\n"])
def test_apply_fixes_codes_counts_and_text(dev, nl):
    rng = np.random.default_rng(9)
    # lower-case bases, a blank inside a sequence line, trailing blanks, a long read, short and empty reads
    seqs = ["ACGTacgtACGTNNAC", "AC GT AC  GTACGT", "acgtacgt \t", "", "A", sc.rand_seq(rng, 3000), "TTTT", "GGGGCC"]
    recs = [("r%d" % i, s) for i, s in enumerate(seqs)]
    quals = ["".join(chr(33 + int(x)) for x in rng.integers(0, 60, len(s))).replace("@", "I") for s in seqs]
    text = _fastq(recs, nl, quals)
    off = rc.fastq_offsets(text)
    kept = [(n, "".join(s.split(" ")).rstrip()) for n, s in recs]  # what the parser keeps
    codes, rec_seq, n = sc.codes_of(kept)
    assert len(off) == len(recs) + 1
    fix = np.full(n, NOFIX, np.uint8)
    at = [0, 5, 15, 16, 18, 21, 31, 32, 39, 40, rec_seq[5], rec_seq[5] + 1023, rec_seq[5] + 1024, rec_seq[5] + 2999,
          n - 1, n - 7]
    for i, b in enumerate(at):
        fix[int(b)] = (int(codes[int(b)]) + 1 + i % 3) & 3
    want_codes = cc.apply_codes(codes[:n].tolist(), fix.tolist())
    want_n = cc.nfix(fix.tolist(), rec_seq, n)
    want_text = cc.apply_text(text, off, rec_seq, fix.tolist(), n)
    assert want_text != text and len(want_text) == len(text) and sum(want_n) == len(at)
    assert sum(1 for a, b in zip(text, want_text) if a != b) == len(at)
    for r, rec in enumerate(rc.records_of(want_text, off)):  # the quality line and every other line unchanged
        a, b = rc.record_lines(rec), rc.record_lines(rc.records_of(text, off)[r])
        assert (a[0], a[2], a[3]) == (b[0], b[2], b[3])
    assert want_text[off[0] + 5 + len(nl) + 5:][:1].islower()  # base 5 replaces a lower-case letter
    rc_, got_codes, got_n, got_text = _apply(dev, codes, fix, rec_seq, n, text, off)
    assert rc_ == N.KMAN_OK, N.lib().kman_last_error(dev.ctx)
    assert got_codes[:n].tolist() == want_codes and np.all(got_codes[n:] == 4)
    assert got_n[:len(recs)].tolist() == want_n and np.all(got_n[len(recs):] == 0xA5A5A5A5)
    assert got_text[:len(text)] == want_text and got_text[len(text):] == bytes([SENT]) * PAD
    # without a text: the same codes and counts
    rc_, got_codes, got_n, _ = _apply(dev, codes, fix, rec_seq, n)
    assert rc_ == N.KMAN_OK and got_codes[:n].tolist() == want_codes and got_n[:len(recs)].tolist() == want_n
    # no fix at all: nothing changes
    rc_, got_codes, got_n, got_text = _apply(dev, codes, np.full(n, NOFIX, np.uint8), rec_seq, n, text, off)
    assert rc_ == N.KMAN_OK and got_codes.tolist() == codes.tolist() and not got_n[:len(recs)].any()
    assert got_text[:len(text)] == text
    # refused: nothing written
    for null in (0, 1, 2, 3, 5):
        rc_, got_codes, got_n, got_text = _apply(dev, codes, fix, rec_seq, n, text, off, null=null)
        assert rc_ == N.KMAN_EINVAL, null
        assert got_codes.tolist() == codes.tolist() and np.all(got_n == 0xA5A5A5A5) and got_text[:len(text)] == text


# ------------------------------------------------------------------ engine API


def _table_of(dev, text, k, canonical):
    from kman_amd import engine

    p = engine.parse(dev, text)
    try:
        table = engine.join_groups(p, k, False, "count", canonical=canonical)
    finally:
        p.free()
    return table


def _reads_case(k, seed=21):
    """Reads of a genome that the table holds three times, with errors of every kind of the rule."""
    g = _genome(600, seed)
    reads = [("r%d" % i, g[30 * i:30 * i + 150]) for i in range(15)]
    for i, at in ((1, 75), (2, 0), (3, 149), (4, k - 1), (5, 150 - k), (6, 40)):
        reads[i] = (reads[i][0], cc.sub(reads[i][1], at, 1 + i % 3))
    reads[6] = (reads[6][0], cc.sub(reads[6][1], 40 + k + 5))        # two errors more than k apart
    reads[7] = (reads[7][0], cc.sub(cc.sub(reads[7][1], 60), 60 + k))  # exactly k apart: left alone
    reads[8] = (reads[8][0], sc.with_n(cc.sub(reads[8][1], 60), [(60 + k, 60 + k + 1)]))
    reads += [("short", g[:k - 1]), ("empty", ""), ("novel", _genome(150, seed + 1))]
    genome = [("g%d" % i, g) for i in range(3)]
    return genome, reads


@pytest.mark.parametrize("canonical", [False, True])
def test_engine_correct(dev, canonical):
    from kman_amd import engine

    k, C = 21, 3
    genome, reads = _reads_case(k)
    table = sc.table_of(genome, k, canonical)
    fix = cc.fix_plane_of(reads, k, table, C, canonical)
    codes, rec_seq, n = sc.codes_of(reads)
    want_n = cc.nfix(fix, rec_seq, n)
    assert want_n[:9] == [0, 1, 1, 1, 1, 1, 2, 0, 0] and sum(want_n) == 7
    text = _fastq(reads)
    dtab = _table_of(dev, sc.fasta(genome), k, canonical)
    p = engine.parse(dev, text, keep_text=True)
    try:
        d_wc = engine.window_counts(p, dtab, canonical)
        try:
            before = dev.download(d_wc, n, np.uint32)
        finally:
            d_wc.free()
        got = engine.correct(p, dtab, canonical, C)
        assert got.dtype == np.uint32 and got.tolist() == want_n
        assert dev.download(p.codes, n, np.uint8).tolist() == cc.apply_codes(codes[:n].tolist(), fix)
        want_text = cc.apply_text(text, rc.fastq_offsets(text), rec_seq, fix, n)
        assert dev.download(p.text, len(text), np.uint8).tobytes() == want_text
        # every window of a corrected run is solid now, and no record has fewer solid windows than before
        d_wc = engine.window_counts(p, dtab, canonical)
        try:
            after = dev.download(d_wc, n, np.uint32)
            # a second pass finds nothing more to do in the repaired reads: the words are given, not recomputed
            assert engine.correct(p, dtab, canonical, C, d_wc=d_wc).tolist()[:6] == [0] * 6
        finally:
            d_wc.free()
        fixed = cc.corrected(reads, fix)
        assert after.tolist() == mc.window_words(fixed, k, table, canonical)
        rs = list(rec_seq) + [n]
        for r in range(len(reads)):
            b, a = before[int(rs[r]):int(rs[r + 1])], after[int(rs[r]):int(rs[r + 1])]
            assert sum(so.solid(x, C) for x in a) >= sum(so.solid(x, C) for x in b), r
        for pos in [i for i, f in enumerate(fix) if f != NOFIX]:
            r = int(np.searchsorted(rec_seq, pos, side="right")) - 1
            lo, hi = max(int(rs[r]), pos - k + 1), min(pos, int(rs[r + 1]) - k)
            assert all(so.solid(x, C) for x in after[lo:hi + 1]), pos
    finally:
        p.free()
    # without the text, with the caller's index, FASTA input: the same counts
    idx = engine.table_index(dev, dtab, 4)
    p = engine.parse(dev, sc.fasta(reads))
    try:
        assert engine.correct(p, dtab, canonical, C, index=idx, index_bits=4).tolist() == want_n
        for bad in (0, -1, 0xFFFFFFFF, 1.5, True, None):
            with pytest.raises(AssertionError):
                engine.correct(p, dtab, canonical, bad)
    finally:
        p.free()
        idx.free()
        engine.free_result(dtab)


# ------------------------------------------------------------------------ CLI


def _cli(*argv):
    from kman_amd.scripts.kmer import main

    r = CliRunner().invoke(main, [str(a) for a in argv], catch_exceptions=False)
    assert r.exit_code == 0, r.output


def _cli_inputs(tmp_path, k):
    genome, reads = _reads_case(k, seed=22)
    rng = np.random.default_rng(5)
    quals = ["".join(chr(33 + int(x)) for x in rng.integers(25, 31, len(s))) for _, s in reads]
    quals[1] = quals[1][:75 + k] + "#" + quals[1][75 + k + 1:]  # -q 20 masks a base right after read 1's weak run
    quals[9] = quals[9][:10] + "!" + quals[9][11:]
    text = _fastq(reads, quals=quals)
    (tmp_path / "reads.fq").write_bytes(text)
    with gzip.open(tmp_path / "reads.fq.gz", "wb") as fh:
        fh.write(text)
    (tmp_path / "reads.fa").write_bytes(sc.fasta(reads))
    (tmp_path / "genome.fa").write_bytes(sc.fasta(genome))
    return genome, reads, text


@pytest.mark.parametrize("canonical, q", [(False, 0), (True, 20)])
def test_cli_correct_end_to_end(tmp_path, canonical, q):
    """The TSV with FIXES, --bed, --reads-out with and without --trim; plain FASTQ, and gzipped FASTQ with -q 20."""
    from fastq_qual_cases import mask_fastq

    k, C = 21, 3
    genome, reads, text = _cli_inputs(tmp_path, k)
    out, bed, fq = tmp_path / "out.tsv", tmp_path / "out.bed", tmp_path / "out.fq"
    off = rc.fastq_offsets(text)
    flags = (["--canonical"] if canonical else []) + (["-q", q] if q else [])
    table = sc.table_of(genome, k, canonical)
    masked = sc.fasta_records(mask_fastq(text, q, 33)[0]) if q else reads
    fixed, stats, span, fixes = cc.screen_of(masked, k, table, C, canonical)
    assert sum(fixes) == (6 if q else 7) and fixes[1] == (0 if q else 1)
    fix = cc.fix_plane_of(masked, k, table, C, canonical)
    _, rec_seq, n = sc.codes_of(masked)
    want_text = cc.apply_text(text, off, rec_seq, fix, n)
    src = tmp_path / ("reads.fq.gz" if q else "reads.fq")
    _cli("screen", src, tmp_path / "genome.fa", out, k, "--solid", C, "--correct", "--bed", bed, "--reads-out", fq,
         *flags)
    assert out.read_bytes() == cc.lines(masked, stats, span, fixes)
    assert bed.read_bytes() == so.bed(masked, span)
    assert fq.read_bytes() == want_text
    _cli("screen", src, tmp_path / "genome.fa", out, k, "--solid", C, "--correct", "--reads-out", fq, "--trim",
         "--median", *flags)
    assert out.read_bytes() == cc.lines(masked, stats, span, fixes, mc.medians(fixed, k, table, canonical))
    assert fq.read_bytes() == rc.cut_trimmed(want_text, off, [a for a, _ in span], [b for _, b in span])


def test_cli_selection_fasta_and_todays_bytes(tmp_path):
    k, C = 21, 3
    genome, reads, text = _cli_inputs(tmp_path, k)
    out, bed, fq = tmp_path / "out.tsv", tmp_path / "out.bed", tmp_path / "out.fq"
    off = rc.fastq_offsets(text)
    table = sc.table_of(genome, k, True)
    fixed, stats, span, fixes = cc.screen_of(reads, k, table, C, True)
    plain_stats = sc.stats(reads, k, table, True)
    plain_span = so.spans(so.runs_of(reads, k, table, C, True), k)
    # a selection reads the corrected records: the repaired reads have their whole length again
    kept = so.keep(stats, span, min_solid_len=150)
    assert sum(kept) > sum(so.keep(plain_stats, plain_span, min_solid_len=150))
    _cli("screen", tmp_path / "reads.fq", tmp_path / "genome.fa", out, k, "--canonical", "--solid", C, "--correct",
         "--min-solid-len", 150)
    assert out.read_bytes() == cc.lines(reads, stats, span, fixes, kept=kept)
    # FASTA READS without --reads-out
    _cli("screen", tmp_path / "reads.fa", tmp_path / "genome.fa", out, k, "--canonical", "--solid", C, "--correct")
    assert out.read_bytes() == cc.lines(reads, stats, span, fixes)
    # without --correct: the bytes of the same command before the option existed
    _cli("screen", tmp_path / "reads.fq", tmp_path / "genome.fa", out, k, "--canonical", "--solid", C, "--bed", bed,
         "--reads-out", fq, "--trim")
    assert out.read_bytes() == so.lines(reads, plain_stats, plain_span)
    assert bed.read_bytes() == so.bed(reads, plain_span)
    assert fq.read_bytes() == rc.cut_trimmed(text, off, [a for a, _ in plain_span], [b for _, b in plain_span])
    _cli("screen", tmp_path / "reads.fq", tmp_path / "genome.fa", out, k, "--canonical", "--reads-out", fq)
    assert out.read_bytes() == sc.lines(reads, plain_stats) and fq.read_bytes() == rc.cut_whole(text, off)
