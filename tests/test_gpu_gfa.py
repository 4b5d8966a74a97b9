"""The edges between unitigs on the GPU: kman_unitig_edges on its own (keys
from the Python table, the index from kman_table_index, the rank arrays from
the plain-Python statement), engine.unitigs(links=True) and `kmer unitigs
--gfa`, all against tests/gfa_cases.py for equality."""

from __future__ import annotations

import gzip
from ctypes import byref, c_double, c_uint64, c_void_p

import numpy as np
import pytest
from click.testing import CliRunner

import gfa_cases as gc
import hpc_cases as hc
import screen_cases as sc
import unitig_cases as uc

pytestmark = pytest.mark.gpu

from kman_amd import _native as N  # noqa: E402

PAD = 16  # sentinel words after an output
SENT32, SENT64 = 0xA5A5A5A5, 0xA5A5A5A5A5A5A5A5
CASES = uc.cases()
TILE_CASES = gc.tile_cases(N.KMAN_EDGE_TILE)


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
        return self.up(np.full(n + PAD, SENT32 if np.dtype(dtype).itemsize == 4 else SENT64, dtype))

    def free(self):
        for b in self.all:
            b.free()


class _Table:
    """A table's inputs on the device and what the statement expects."""

    def __init__(self, dev, table, k, bits=None):
        from kman_amd import engine

        self.dev, self.k, self.bufs = dev, k, _Bufs(dev)
        self.keys, _ = sc.table_rows(table)
        self.n = len(self.keys)
        self.ranks = uc.rank_arrays(table)
        self.units, self.edges = gc.table_edges(table, k)
        self.U, self.E = len(self.units), len(self.edges)
        self.eoff, self.words = gc.csr(self.edges, self.U)
        self.d_keys = self.bufs.up(self.keys)
        self.d_ranks = [self.bufs.up(r) for r in self.ranks]
        self.set_bits(engine.default_index_bits(self.n, k) if bits is None else bits)

    def set_bits(self, bits):
        self.bits = bits
        self.d_index = self.bufs.sent((1 << bits) + 1, np.uint64)
        assert N.lib().kman_table_index(self.dev.ctx, c_void_p(self.d_keys.ptr), self.n, self.k, bits,
                                        c_void_p(self.d_index.ptr)) == N.KMAN_OK
        self.index = self.dev.download(self.d_index, (1 << bits) + 1, np.uint64)

    def call(self, caps=None, want_rc=N.KMAN_OK, outputs=(1, 1), k=None, bits=None, nt=None, null=None):
        """kman_unitig_edges into sentinel-filled buffers of `caps` (2 U, E by
        default); returns (rc, n_ends, n_edges, eoff, edge) and checks that
        nothing lies past the outputs and that a refused call wrote nothing."""
        ecap, wcap = caps if caps is not None else (2 * self.U, self.E)
        d_eoff, d_edge = self.bufs.sent(ecap + 1, np.uint64), self.bufs.sent(wcap, np.uint32)
        ins = {"keys": self.d_keys, "index": self.d_index, "start": self.d_ranks[0], "pos": self.d_ranks[1],
               "nodes": self.d_ranks[2]}
        ptr = {name: (None if name == null else c_void_p(b.ptr)) for name, b in ins.items()}
        ne, nw = c_uint64(77), c_uint64(77)
        rc = N.lib().kman_unitig_edges(self.dev.ctx, ptr["keys"], self.n if nt is None else nt,
                                       self.k if k is None else k, ptr["index"], self.bits if bits is None else bits,
                                       ptr["start"], ptr["pos"], ptr["nodes"],
                                       c_void_p(d_eoff.ptr) if outputs[0] else None, ecap,
                                       c_void_p(d_edge.ptr) if outputs[1] else None, wcap, byref(ne), byref(nw))
        assert rc == want_rc, N.lib().kman_last_error(self.dev.ctx)
        eoff = self.dev.download(d_eoff, ecap + 1 + PAD, np.uint64)
        edge = self.dev.download(d_edge, wcap + PAD, np.uint32)
        if rc != N.KMAN_OK or not all(outputs):
            assert np.all(eoff == np.uint64(SENT64)) and np.all(edge == np.uint32(SENT32))  # nothing written
            return rc, ne.value, nw.value, None, None
        n_ends, n_edges = int(ne.value), int(nw.value)
        assert np.all(eoff[n_ends + 1:] == np.uint64(SENT64)) and np.all(edge[n_edges:] == np.uint32(SENT32))
        return rc, n_ends, n_edges, eoff[:n_ends + 1], edge[:n_edges]

    def check(self):
        """The sizing call, the filling call at exactly 2 U and E, twice, and
        the inputs afterwards."""
        rc, n_ends, n_edges, _, _ = self.call(outputs=(0, 0))
        assert (n_ends, n_edges) == (2 * self.U, self.E)
        rc, n_ends, n_edges, eoff, edge = self.call()
        assert (n_ends, n_edges) == (2 * self.U, self.E)
        np.testing.assert_array_equal(eoff, self.eoff)
        np.testing.assert_array_equal(edge, self.words)
        again = self.call()
        assert again[3].tobytes() == eoff.tobytes() and again[4].tobytes() == edge.tobytes()
        np.testing.assert_array_equal(self.dev.download(self.d_keys, self.n, np.uint64), self.keys)
        np.testing.assert_array_equal(self.dev.download(self.d_index, (1 << self.bits) + 1, np.uint64), self.index)
        for d, w in zip(self.d_ranks, self.ranks):
            np.testing.assert_array_equal(self.dev.download(d, self.n, np.uint32), w)

    def free(self):
        self.bufs.free()


def _every_index_width(dev, table, k):
    from kman_amd import engine

    t = _Table(dev, table, k)
    try:
        for bits in sorted({1, engine.default_index_bits(t.n, k), min(2 * k, N.KMAN_SCREEN_MAX_INDEX_BITS)}):
            t.set_bits(bits)
            t.check()
        return t.U, t.E
    finally:
        t.free()


@pytest.mark.parametrize("name", sorted(n for n in CASES if n != "empty"))  # (no rows: test_empty_table)
def test_edges_alone_on_every_case(dev, name):
    records, k, min_count = CASES[name]
    got = {_every_index_width(dev, uc.table_of(records, k, min_count), k),
           _every_index_width(dev, uc.table_of(uc.both_strands(records), k, 2 * min_count - 1), k)}
    assert len(got) == 1


@pytest.mark.parametrize("name", sorted(TILE_CASES))
def test_edges_alone_at_tile_edges(dev, name):
    records, k, min_count = TILE_CASES[name]
    U, E = _every_index_width(dev, uc.table_of(records, k, min_count), k)
    assert 2 * U == int(name.split("_")[1]) and E > 0


def test_capacities_and_refusals(dev):
    records, k, _ = CASES["all_5mers"]
    t = _Table(dev, uc.table_of(records, k), k)
    try:
        U, E = t.U, t.E
        assert E == 8 * U  # every end full: the bound is met exactly
        rc, n_ends, n_edges, eoff, edge = t.call(caps=(2 * U, 8 * U))
        np.testing.assert_array_equal(eoff, t.eoff)
        np.testing.assert_array_equal(edge, t.words)
        for caps in ((2 * U - 1, E), (2 * U, E - 1), (0, 0)):
            rc, n_ends, n_edges, _, _ = t.call(caps=caps, want_rc=N.KMAN_ECAP)
            assert (n_ends, n_edges) == (2 * U, E)  # the sizes it needs
        rc, n_ends, n_edges, eoff, edge = t.call(caps=(2 * U + 5, E + 9))  # room to spare
        np.testing.assert_array_equal(eoff, t.eoff)
        np.testing.assert_array_equal(edge, t.words)
    finally:
        t.free()
    records, k, _ = CASES["y_fork"]
    t = _Table(dev, uc.table_of(records, k), k, bits=6)
    try:
        for outputs in ((1, 0), (0, 1)):
            t.call(want_rc=N.KMAN_EINVAL, outputs=outputs)
        for bad_k in (20, 33, 1, 2, 32):
            t.call(want_rc=N.KMAN_EINVAL, k=bad_k)
        for bad_bits in (0, 25):
            t.call(want_rc=N.KMAN_EINVAL, bits=bad_bits)
        t.call(want_rc=N.KMAN_EINVAL, k=3, bits=7)  # more index bits than 2 k
        t.call(want_rc=N.KMAN_EINVAL, nt=N.KMAN_GRAPH_MAX_ROWS)
        for null in ("keys", "index", "start", "pos", "nodes"):
            t.call(want_rc=N.KMAN_EINVAL, null=null)
        t.check()  # the context is still usable
    finally:
        t.free()


def test_empty_table(dev, tmp_path):
    from kman_amd import engine

    L = N.lib()
    bufs = _Bufs(dev)
    try:
        d_eoff, d_edge = bufs.sent(1, np.uint64), bufs.sent(0, np.uint32)
        ne, nw = c_uint64(9), c_uint64(9)
        assert L.kman_unitig_edges(dev.ctx, None, 0, 21, None, 4, None, None, None, None, 0, None, 0, byref(ne),
                                   byref(nw)) == N.KMAN_OK
        assert (ne.value, nw.value) == (0, 0)
        ne, nw = c_uint64(9), c_uint64(9)
        assert L.kman_unitig_edges(dev.ctx, None, 0, 21, None, 4, None, None, None, c_void_p(d_eoff.ptr), 0,
                                   c_void_p(d_edge.ptr), 0, byref(ne), byref(nw)) == N.KMAN_OK
        assert (ne.value, nw.value) == (0, 0)
        eoff = dev.download(d_eoff, 1 + PAD, np.uint64)
        assert eoff[0] == 0 and np.all(eoff[1:] == np.uint64(SENT64))  # d_eoff[0] = 0 and nothing else
        assert np.all(dev.download(d_edge, PAD, np.uint32) == np.uint32(SENT32))
    finally:
        bufs.free()
    t = engine.empty_count(dev, 21)
    try:
        r = engine.unitigs(dev, t, links=True)
        plain = engine.unitigs(dev, t)
    finally:
        engine.free_result(t)
    assert r.n == 0 and list(r.eoff) == [0] and len(r.edges) == 0 and engine.emit_gfa(r) == b"H\tVN:Z:1.0\n"
    assert plain.eoff is None and plain.edges is None
    src, out = tmp_path / "in.fa", tmp_path / "out.gfa"
    src.write_bytes(b">short\nACGTNNNNACGT\n")
    _cli("unitigs", src, out, 21, "--gfa")
    assert out.read_bytes() == b"H\tVN:Z:1.0\n"


def test_foreign_index_and_ranks_stay_in_bounds(dev):
    """Bounds, not values: these calls return and write nothing past their
    outputs; what they write is not checked beyond that."""
    records, k, _ = CASES["two_cycles_and_paths"]
    t = _Table(dev, uc.table_of(records, k), k, bits=8)
    rng = np.random.default_rng(5)
    try:
        n = t.n
        own_index, own_ranks, own_keys = t.d_index, t.d_ranks, t.d_keys
        foreign = (rng.integers(0, 1 << 62, (1 << 8) + 1, dtype=np.uint64) * np.uint64(7)).astype(np.uint64)
        foreign[::3] = np.uint64(SENT64)
        d_foreign, d_desc = t.bufs.up(foreign), t.bufs.up(t.keys[::-1].copy())
        wild = [t.bufs.up(rng.integers(0, top, n, dtype=np.uint64).astype(np.uint32)) for top in (2 * n, 4, 1000)]
        junk = [t.bufs.up(rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)) for _ in range(3)]
        for keys, index, ranks in ((own_keys, d_foreign, own_ranks), (d_desc, own_index, own_ranks),
                                   (d_desc, d_foreign, wild), (own_keys, own_index, wild),
                                   (own_keys, own_index, junk)):
            t.d_keys, t.d_index, t.d_ranks = keys, index, ranks
            rc, n_ends, n_edges, _, _ = t.call(outputs=(0, 0))
            assert n_ends <= 2 * n and n_edges <= 4 * n_ends
            # (rows that claim one end race: the edges of two calls may differ, the ends do not)
            rc, n_ends2, n_edges, eoff, edge = t.call(caps=(n_ends, 4 * n_ends))
            assert n_ends2 == n_ends and int(eoff[-1]) == n_edges
            assert np.all(np.diff(eoff.astype(np.int64)) >= 0) and np.all(edge >> 1 < max(1, n_ends // 2))
        t.d_keys, t.d_index, t.d_ranks = own_keys, own_index, own_ranks
        t.check()
    finally:
        t.free()


def test_launches_are_timed(dev):
    L = N.lib()
    records, k, _ = CASES["cycle_with_tail"]
    t = _Table(dev, uc.table_of(records, k), k)
    assert L.kman_timing_enable(dev.ctx, 1) == N.KMAN_OK
    try:
        t.call()
        m, ms = c_uint64(0), c_double(0)
        assert L.kman_timing_query(dev.ctx, b"unitig_edges", byref(m), byref(ms)) == N.KMAN_OK
        assert m.value >= 3 and ms.value > 0
    finally:
        L.kman_timing_enable(dev.ctx, 0)
        t.free()


# ------------------------------------------------------- engine and command


def _device_table(dev, text, k, min_count=1, fastq=False, hpc=False):
    from kman_amd import engine

    p = engine.parse_fastq(dev, text) if fastq else engine.parse(dev, text)
    if hpc:
        p = engine.hpc(p)
    try:
        t = engine.join_groups(p, k, False, "count", canonical=True)
    finally:
        p.free()
    if min_count > 1:
        ranged = engine.filtered_copy(dev, t, min_count)
        engine.free_result(t)
        t = ranged
    return t


def _engine(dev, t, table, k, index_bits=None):
    from kman_amd import engine

    try:
        assert int(t.n) == len(table)
        r = engine.unitigs(dev, t, index_bits=index_bits, links=True)
        plain = engine.unitigs(dev, t, index_bits=index_bits)
    finally:
        engine.free_result(t)
    units, edges = gc.table_edges(table, k)
    assert [(r.seq(u), int(r.nodes[u]), int(r.kc[u])) for u in range(r.n)] == units
    eoff, words = gc.csr(edges, len(units))
    np.testing.assert_array_equal(r.eoff, eoff)
    np.testing.assert_array_equal(r.edges, words)
    assert r.eoff.dtype == np.uint64 and r.edges.dtype == np.uint32
    assert engine.emit_gfa(r) == gc.gfa_text(units, edges, k)
    assert plain.eoff is None and plain.edges is None  # links=False: as before
    assert engine.emit_unitigs(plain) == engine.emit_unitigs(r) == uc.text(units)
    with pytest.raises(AssertionError):
        engine.emit_gfa(plain)


@pytest.mark.parametrize("name", ["y_fork", "fork_and_merge", "all_3mers", "two_cycles_and_paths", "acgt_k3",
                                  "tip_removed_by_L2", "tip_kept", "poly_a_with_neighbours", "ends_770"])
def test_engine_links(dev, name):
    records, k, min_count = CASES[name] if name in CASES else TILE_CASES[name]
    table = uc.table_of(records, k, min_count)
    _engine(dev, _device_table(dev, sc.fasta(records), k, min_count), table, k)
    if name == "two_cycles_and_paths":
        _engine(dev, _device_table(dev, sc.fasta(records), k, min_count), table, k, index_bits=1)


def test_engine_links_fastq_hpc(dev):
    import fastq_cases as fq

    k = 11
    qtext = fq.mixed_reads(seed=12, n_records=80)
    reads = sc.fasta_records(fq.fastq_to_fasta(qtext))
    squeezed = [(n, hc.hpc_seq(s)[0]) for n, s in reads]
    _engine(dev, _device_table(dev, qtext, k, fastq=True, hpc=True), uc.table_of(squeezed, k), k)


def _cli(*argv, ok=True):
    from kman_amd.scripts.kmer import main

    r = CliRunner().invoke(main, [str(a) for a in argv], catch_exceptions=not ok)
    if ok:
        assert r.exit_code == 0, r.output
    return r


def test_cli_gfa(tmp_path):
    import fastq_cases as fq

    for name in ("fork_and_merge", "cycle_with_tail", "tip_removed_by_L2"):
        records, k, min_count = CASES[name]
        units, edges = gc.table_edges(uc.table_of(records, k, min_count), k)
        src, out, fa = tmp_path / (name + ".fa"), tmp_path / (name + ".gfa"), tmp_path / (name + ".out.fa")
        src.write_bytes(sc.fasta(records))
        argv = ["-L", min_count] if min_count > 1 else []
        _cli("unitigs", src, out, k, "--gfa", *argv)
        assert out.read_bytes() == gc.gfa_text(units, edges, k)
        parsed = gc.parse_gfa(out.read_bytes())
        assert parsed[0] == [(s, kc) for s, _, kc in units] and parsed[1] == edges
        _cli("unitigs", src, fa, k, *argv)
        assert fa.read_bytes() == uc.text(units)  # without the flag: the text as before
        r = _cli("unitigs", src, str(out) + ".gz", k, "--gfa", ok=False)
        assert isinstance(r.exception, AssertionError) and "ends in .gz" in str(r.exception)
        assert not (tmp_path / (name + ".gfa.gz")).exists()
    k = 11
    qtext = fq.mixed_reads(seed=12, n_records=80)
    reads = sc.fasta_records(fq.fastq_to_fasta(qtext))
    fqgz, out = tmp_path / "reads.fq.gz", tmp_path / "reads.gfa"
    with gzip.open(fqgz, "wb") as fh:
        fh.write(qtext)
    squeezed = [(n, hc.hpc_seq(s)[0]) for n, s in reads]
    for argv, recs, kw in (([], reads, {}), (["--hpc", "-L", 2, "--index-bits", 1], squeezed, {"min_count": 2})):
        _cli("unitigs", fqgz, out, k, "--gfa", *argv)
        units, edges = gc.table_edges(uc.table_of(recs, k, **kw), k)
        assert out.read_bytes() == gc.gfa_text(units, edges, k)
