"""Unitigs of a count table on the GPU: kman_graph_links, kman_graph_rank and
kman_unitig_spell each on its own, engine.unitigs and `kmer unitigs`, all
against the plain-Python statement (tests/unitig_cases.py) for equality."""

from __future__ import annotations

import gzip
from ctypes import byref, c_uint32, c_uint64, c_void_p

import numpy as np
import pytest
from click.testing import CliRunner

import hpc_cases as hc
import screen_cases as sc
import unitig_cases as uc

pytestmark = pytest.mark.gpu

from kman_amd import _native as N  # noqa: E402

PAD = 16  # sentinel words after an output
SENT32, SENT64, SENT8 = 0xA5A5A5A5, 0xA5A5A5A5A5A5A5A5, 0xA5
CASES = uc.cases()


@pytest.fixture(scope="module")
def dev():
    from kman_amd import engine

    return engine.default_device()


class _Bufs:
    """Device buffers freed together."""

    def __init__(self, dev):
        self.dev, self.all = dev, []

    def up(self, arr):
        arr = np.ascontiguousarray(arr)
        buf = self.dev.alloc(max(16, arr.nbytes))
        if arr.nbytes:
            self.dev.upload(buf, arr)
        self.all.append(buf)
        return buf

    def sent(self, n, dtype):
        fill = {4: SENT32, 8: SENT64, 1: SENT8}[np.dtype(dtype).itemsize]
        return self.up(np.full(n + PAD, fill, dtype))

    def free(self):
        for b in self.all:
            b.free()


def _index(dev, bufs, d_keys, n, k, bits):
    d_index = bufs.sent((1 << bits) + 1, np.uint64)
    assert N.lib().kman_table_index(dev.ctx, c_void_p(d_keys.ptr), n, k, bits, c_void_p(d_index.ptr)) == N.KMAN_OK
    return d_index


def _links(dev, bufs, d_keys, n, k, d_index, bits, want_rc=N.KMAN_OK, nt=None):
    d_link = bufs.sent(2 * n, np.uint32)
    rc = N.lib().kman_graph_links(dev.ctx, c_void_p(d_keys.ptr) if d_keys else None, n if nt is None else nt, k,
                                  c_void_p(d_index.ptr) if d_index else None, bits, c_void_p(d_link.ptr))
    assert rc == want_rc, N.lib().kman_last_error(dev.ctx)
    got = dev.download(d_link, 2 * n + PAD, np.uint32)
    assert np.all(got[2 * n:] == SENT32)
    if rc != N.KMAN_OK:
        assert np.all(got == SENT32)  # a refused call writes nothing
    return d_link, got[:2 * n]


def _rank(dev, bufs, d_link, n, want_rc=N.KMAN_OK, nt=None):
    outs = [bufs.sent(n, np.uint32) for _ in range(3)]
    rounds, cycles = c_uint32(77), c_uint64(77)
    rc = N.lib().kman_graph_rank(dev.ctx, c_void_p(d_link.ptr) if d_link else None, n if nt is None else nt,
                                 *[c_void_p(o.ptr) for o in outs], byref(rounds), byref(cycles))
    assert rc == want_rc, N.lib().kman_last_error(dev.ctx)
    got = [dev.download(o, n + PAD, np.uint32) for o in outs]
    for g in got:
        assert np.all(g[n:] == SENT32)
        if rc != N.KMAN_OK:
            assert np.all(g == SENT32)
    return outs, [g[:n] for g in got], rounds.value, cycles.value


def _spell(dev, bufs, d_keys, d_counts, cb, n, k, ranks, caps=None, want_rc=N.KMAN_OK, outputs=(1, 1, 1, 1)):
    """The sizing call, then the filling one into sentinel-filled buffers of
    exactly the sizes it asked for (or `caps`)."""
    L = N.lib()
    nu, nb = c_uint64(0), c_uint64(0)
    args = [dev.ctx, c_void_p(d_keys.ptr), c_void_p(d_counts.ptr), cb, n, k] + [c_void_p(r.ptr) for r in ranks]
    rc = L.kman_unitig_spell(*args, None, None, None, 0, None, 0, byref(nu), byref(nb))
    if want_rc == N.KMAN_EINVAL and rc == N.KMAN_EINVAL:
        U = B = 4
    else:
        assert rc == N.KMAN_OK, L.kman_last_error(dev.ctx)
        U, B = int(nu.value), int(nb.value)
    ucap, scap = caps if caps is not None else (U, B)
    sizes = ((ucap + 1, np.uint64), (ucap, np.uint32), (ucap, np.uint64), (scap, np.uint8))
    outs = [bufs.sent(m, dt) for m, dt in sizes]
    ptrs = [c_void_p(o.ptr) if use else None for o, use in zip(outs, outputs)]
    rc = L.kman_unitig_spell(*args, ptrs[0], ptrs[1], ptrs[2], ucap, ptrs[3], scap, byref(nu), byref(nb))
    assert rc == want_rc, L.kman_last_error(dev.ctx)
    got = [dev.download(o, m + PAD, dt) for o, (m, dt) in zip(outs, sizes)]
    for g, (m, dt) in zip(got, sizes):
        fill = g.dtype.type({4: SENT32, 8: SENT64, 1: SENT8}[g.dtype.itemsize])
        if rc != N.KMAN_OK:
            assert np.all(g == fill)  # a refused call writes nothing
    if rc != N.KMAN_OK:
        return rc, int(nu.value), int(nb.value), None
    off, un, kc, seq = got
    assert int(nu.value) == U and int(nb.value) == B
    assert np.all(off[U + 1:] == np.uint64(SENT64)) and np.all(un[U:] == np.uint32(SENT32))
    assert np.all(kc[U:] == np.uint64(SENT64)) and np.all(seq[B:] == np.uint8(SENT8))
    return rc, U, B, (off[:U + 1], un[:U], kc[:U], seq[:B])


def _want_spell(table):
    units = uc.unitigs(table)
    off = np.cumsum([0] + [len(s) for s, _, _ in units]).astype(np.uint64)
    un = np.asarray([m for _, m, _ in units], dtype=np.uint32)
    kc = np.asarray([c for _, _, c in units], dtype=np.uint64)
    seq = np.frombuffer("".join(s for s, _, _ in units).encode(), dtype=np.uint8)
    return off, un, kc, seq


def _abi(dev, table, k, bits=None, cb=4):
    """Every ABI call on its own on the rows of `table`."""
    from kman_amd import engine

    keys, counts = sc.table_rows(table, cb)
    n = len(keys)
    bits = engine.default_index_bits(n, k) if bits is None else bits
    bufs = _Bufs(dev)
    try:
        d_keys, d_counts = bufs.up(keys), bufs.up(counts)
        d_index = _index(dev, bufs, d_keys, n, k, bits)
        index = dev.download(d_index, (1 << bits) + 1, np.uint64)
        want_link = uc.link_array(table)
        d_link, link = _links(dev, bufs, d_keys, n, k, d_index, bits)
        np.testing.assert_array_equal(link, want_link)
        assert _links(dev, bufs, d_keys, n, k, d_index, bits)[1].tobytes() == link.tobytes()  # twice: equal bytes
        ranks, got, rounds, cycles = _rank(dev, bufs, d_link, n)
        for g, w in zip(got, uc.rank_arrays(table)):
            np.testing.assert_array_equal(g, w)
        walks, want_cycles = uc.walks(table)
        assert cycles == want_cycles
        if want_cycles == 0 and n:
            longest = max(len(w) for w in walks)
            assert rounds == (0 if longest <= 2 else (longest - 2).bit_length())  # ceil(log2(longest - 1))
        again = _rank(dev, bufs, d_link, n)
        assert [g.tobytes() for g in again[1]] == [g.tobytes() for g in got] and again[2:] == (rounds, cycles)
        np.testing.assert_array_equal(dev.download(d_link, 2 * n, np.uint32), want_link)  # the links are not written
        rc, U, B, outs = _spell(dev, bufs, d_keys, d_counts, cb, n, k, ranks)
        want = _want_spell(table)
        assert U == len(want[1]) and B == len(want[3])
        if n:
            for g, w in zip(outs, want):
                np.testing.assert_array_equal(g, w)
            twice = _spell(dev, bufs, d_keys, d_counts, cb, n, k, ranks)[3]
            assert [g.tobytes() for g in twice] == [g.tobytes() for g in outs]
        # no input was written
        np.testing.assert_array_equal(dev.download(d_keys, n, np.uint64), keys)
        np.testing.assert_array_equal(dev.download(d_counts, n, counts.dtype), counts)
        np.testing.assert_array_equal(dev.download(d_index, (1 << bits) + 1, np.uint64), index)
        for r, w in zip(ranks, got):
            np.testing.assert_array_equal(dev.download(r, n, np.uint32), w)
        return rounds
    finally:
        bufs.free()


def _device_table(dev, records, k, min_count=1):
    from kman_amd import engine

    p = engine.parse(dev, sc.fasta(records))
    try:
        t = engine.join_groups(p, k, False, "count", canonical=True)
    finally:
        p.free()
    if t is None:
        return engine.empty_count(dev, k)
    if min_count > 1:
        ranged = engine.filtered_copy(dev, t, min_count)
        engine.free_result(t)
        t = ranged
    return t


def _engine(dev, records, k, min_count, table, index_bits=None):
    from kman_amd import engine

    t = _device_table(dev, records, k, min_count)
    try:
        assert int(t.n) == len(table)
        r = engine.unitigs(dev, t, index_bits=index_bits)
    finally:
        engine.free_result(t)
    want = uc.unitigs(table)
    got = [(r.seq(u), int(r.nodes[u]), int(r.kc[u])) for u in range(r.n)]
    assert got == want  # sequences, order, rows and KC
    assert [int(r.off[u + 1] - r.off[u]) for u in range(r.n)] == [len(s) for s, _, _ in want]  # LN
    if table:
        uc.check_cover([s for s, _, _ in got], table, k)
        uc.check_maximal([s for s, _, _ in got], table, k)
    assert engine.emit_unitigs(r) == uc.text(want)
    return r


def _cli(*argv):
    from kman_amd.scripts.kmer import main

    r = CliRunner().invoke(main, [str(a) for a in argv], catch_exceptions=False)
    assert r.exit_code == 0, r.output


@pytest.mark.parametrize("name", sorted(CASES))
def test_case_at_every_level(dev, name, tmp_path):
    records, k, min_count = CASES[name]
    rounds = set()
    for v, recs in enumerate((records, uc.both_strands(records), uc.reverse_strand(records))):
        table = uc.table_of(recs, k, min_count if v != 1 else 2 * min_count - 1)
        assert sorted(table) == sorted(uc.table_of(records, k, min_count))  # the same rows from either strand
        rounds.add(_abi(dev, table, k, cb=8 if v == 1 else 4))
        _engine(dev, recs, k, min_count if v != 1 else 2 * min_count - 1, table)
        if v < 2:
            src, out = tmp_path / ("in%d.fa" % v), tmp_path / ("out%d.fa" % v)
            src.write_bytes(sc.fasta(recs))
            argv = ["-L", min_count if v != 1 else 2 * min_count - 1] if min_count > 1 else []
            _cli("unitigs", src, out, k, *argv)
            assert out.read_bytes() == uc.text(uc.unitigs(table))
    if name.startswith("path_"):
        p = int(name[5:])
        assert rounds == {0 if p <= 2 else (p - 2).bit_length()}


def test_every_round_count_from_0_to_13_occurs():
    got = {0 if p <= 2 else (p - 2).bit_length() for p in uc.PATH_NODES}
    assert got == set(range(14))


def test_single_bucket_index_and_wide_counts(dev):
    """--index-bits 1: one bucket per half of the key space, the longest
    searches; counts past 2^32 in 8-byte counts sum modulo 2^64."""
    records, k, _ = CASES["two_cycles_and_paths"]
    table = uc.table_of(records, k)
    _abi(dev, table, k, bits=1)
    _engine(dev, records, k, 1, table, index_bits=1)
    big = {w: (1 << 63) + 5 for w in table}
    _abi(dev, big, k, cb=8)
    assert any(kc < (1 << 63) for _, m, kc in uc.unitigs(big) if m % 2 == 0)  # a sum that wrapped


def test_empty_table(dev, tmp_path):
    from kman_amd import engine

    L = N.lib()
    bufs = _Bufs(dev)
    try:
        d = bufs.sent(8, np.uint32)
        nu, nb = c_uint64(9), c_uint64(9)
        assert L.kman_graph_links(dev.ctx, None, 0, 21, None, 4, c_void_p(d.ptr)) == N.KMAN_OK
        assert L.kman_graph_rank(dev.ctx, None, 0, c_void_p(d.ptr), c_void_p(d.ptr), c_void_p(d.ptr), None,
                                 None) == N.KMAN_OK
        assert L.kman_unitig_spell(dev.ctx, None, None, 4, 0, 21, None, None, None, c_void_p(d.ptr), c_void_p(d.ptr),
                                   c_void_p(d.ptr), 0, c_void_p(d.ptr), 0, byref(nu), byref(nb)) == N.KMAN_OK
        assert (nu.value, nb.value) == (0, 0)
        assert np.all(dev.download(d, 8 + PAD, np.uint32) == SENT32)  # nt == 0: nothing written
    finally:
        bufs.free()
    t = engine.empty_count(dev, 21)
    try:
        r = engine.unitigs(dev, t)
    finally:
        engine.free_result(t)
    assert r.n == 0 and len(r.seqs) == 0 and list(r.off) == [0] and engine.emit_unitigs(r) == b""
    src, out = tmp_path / "in.fa", tmp_path / "out.fa"
    src.write_bytes(b">short\nACGTNNNNACGT\n")
    _cli("unitigs", src, out, 21)
    assert out.read_bytes() == b""


def test_refusals_leave_every_sentinel(dev):
    records, k, _ = CASES["y_fork"]
    table = uc.table_of(records, k)
    keys, counts = sc.table_rows(table)
    n = len(keys)
    bufs = _Bufs(dev)
    try:
        d_keys, d_counts = bufs.up(keys), bufs.up(counts)
        d_index = _index(dev, bufs, d_keys, n, k, 6)
        for bad_k in (20, 33, 1, 2, 32):
            _links(dev, bufs, d_keys, n, bad_k, d_index, 6, N.KMAN_EINVAL)
        for bad_bits in (0, 25):
            _links(dev, bufs, d_keys, n, k, d_index, bad_bits, N.KMAN_EINVAL)
        _links(dev, bufs, d_keys, n, 3, d_index, 7, N.KMAN_EINVAL)  # more index bits than 2 k
        _links(dev, bufs, d_keys, n, k, d_index, 6, N.KMAN_EINVAL, nt=N.KMAN_GRAPH_MAX_ROWS)
        _links(dev, bufs, None, n, k, d_index, 6, N.KMAN_EINVAL)
        _links(dev, bufs, d_keys, n, k, None, 6, N.KMAN_EINVAL)
        d_link, _ = _links(dev, bufs, d_keys, n, k, d_index, 6)
        _rank(dev, bufs, d_link, n, N.KMAN_EINVAL, nt=N.KMAN_GRAPH_MAX_ROWS)
        _rank(dev, bufs, None, n, N.KMAN_EINVAL)
        ranks = _rank(dev, bufs, d_link, n)[0]
        want = _want_spell(table)
        U, B = len(want[1]), len(want[3])
        for caps in ((U - 1, B), (U, B - 1), (0, 0)):
            rc, nu, nb, _ = _spell(dev, bufs, d_keys, d_counts, 4, n, k, ranks, caps=caps, want_rc=N.KMAN_ECAP)
            assert (nu, nb) == (U, B)  # the sizes it needs
        _spell(dev, bufs, d_keys, d_counts, 4, n, k, ranks, want_rc=N.KMAN_EINVAL, outputs=(1, 1, 0, 1))
        _spell(dev, bufs, d_keys, d_counts, 2, n, k, ranks, want_rc=N.KMAN_EINVAL)
        _spell(dev, bufs, d_keys, d_counts, 4, n, 20, ranks, want_rc=N.KMAN_EINVAL)
        # the context is still usable
        outs = _spell(dev, bufs, d_keys, d_counts, 4, n, k, ranks)[3]
        for g, w in zip(outs, want):
            np.testing.assert_array_equal(g, w)
    finally:
        bufs.free()


def test_foreign_index_and_descending_keys_stay_in_bounds(dev):
    """The lookup's promise: bounds, not values.  Every loop is bounded by a
    count fixed before it starts, so these calls return; what they write is
    not checked beyond the sentinels after the outputs."""
    records, k, _ = CASES["two_cycles_and_paths"]
    keys, counts = sc.table_rows(uc.table_of(records, k))
    n, bits = len(keys), 8
    rng = np.random.default_rng(5)
    bufs = _Bufs(dev)
    try:
        d_keys, d_counts = bufs.up(keys), bufs.up(counts)
        d_desc = bufs.up(keys[::-1].copy())
        d_index = _index(dev, bufs, d_keys, n, k, bits)
        foreign = (rng.integers(0, 1 << 62, (1 << bits) + 1, dtype=np.uint64) * np.uint64(7)).astype(np.uint64)
        foreign[::3] = np.uint64(SENT64)
        d_foreign = bufs.up(foreign)
        for dk, di in ((d_keys, d_foreign), (d_desc, d_index), (d_desc, d_foreign)):
            d_link, link = _links(dev, bufs, dk, n, k, di, bits)
            ok = link != uc.NONE
            assert np.all(link[ok] < 2 * n) and np.all(link[link[ok]] == np.nonzero(ok)[0])  # still symmetric
            ranks = _rank(dev, bufs, d_link, n)[0]
            _spell(dev, bufs, dk, d_counts, 4, n, k, ranks)
        # link words that are no links, rank arrays that are no ranks
        junk = rng.integers(0, 1 << 32, 2 * n, dtype=np.uint64).astype(np.uint32)
        junk[::2] = rng.integers(0, 2 * n, n, dtype=np.uint64).astype(np.uint32)
        ranks = _rank(dev, bufs, bufs.up(junk), n)[0]
        _spell(dev, bufs, d_keys, d_counts, 4, n, k, ranks)
        # (start rows half of them past the table, every second row a head, small node counts: the text stays small)
        wild = [bufs.up(rng.integers(0, top, n, dtype=np.uint64).astype(np.uint32)) for top in (2 * n, 4, 1000)]
        _spell(dev, bufs, d_keys, d_counts, 4, n, k, wild)
    finally:
        bufs.free()


def test_launches_are_timed(dev):
    from ctypes import c_double

    L = N.lib()
    records, k, _ = CASES["cycle_with_tail"]
    table = uc.table_of(records, k)
    assert L.kman_timing_enable(dev.ctx, 1) == N.KMAN_OK
    try:
        _abi(dev, table, k)
        for tag in (b"graph_links", b"graph_rank", b"unitig_spell"):
            m, ms = c_uint64(0), c_double(0)
            assert L.kman_timing_query(dev.ctx, tag, byref(m), byref(ms)) == N.KMAN_OK
            assert m.value >= 2 and ms.value > 0, tag
    finally:
        L.kman_timing_enable(dev.ctx, 0)


def test_cli_formats_and_options(tmp_path):
    import fastq_cases as fq
    from fastq_qual_cases import mask_fastq

    k = 11
    qtext = fq.mixed_reads(seed=12, n_records=80)
    reads = sc.fasta_records(fq.fastq_to_fasta(qtext))
    fa, fqgz, out = tmp_path / "reads.fa", tmp_path / "reads.fq.gz", tmp_path / "out.fa"
    fa.write_bytes(sc.fasta(reads))
    with gzip.open(fqgz, "wb") as fh:
        fh.write(qtext)

    def run(src, records, argv=(), **kw):
        _cli("unitigs", src, out, k, *argv)
        table = uc.table_of(records, k, **kw)
        data = out.read_bytes()
        assert data == uc.text(uc.unitigs(table))
        seqs = [s for s, _, _ in uc.parse_text(data, k)]
        uc.check_cover(seqs, table, k)
        uc.check_maximal(seqs, table, k)
        return data

    plain = run(fa, reads)
    assert run(fqgz, reads) == plain
    assert run(fa, reads, ["--index-bits", 1]) == plain
    assert run(fa, reads, ["--format", "fasta"]) == plain
    assert run(fqgz, reads, ["-L", 2], min_count=2) != plain
    run(fqgz, reads, ["-L", 2, "-U", 3], min_count=2, max_count=3)
    masked = sc.fasta_records(mask_fastq(qtext, 25, 33)[0])
    assert run(fqgz, masked, ["-q", 25]) != plain
    squeezed = [(n, hc.hpc_seq(s)[0]) for n, s in reads]
    assert run(fqgz, squeezed, ["--hpc"]) != plain
    run(fqgz, squeezed, ["--hpc", "-L", 2, "--index-bits", 1], min_count=2)
