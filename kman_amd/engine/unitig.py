"""Maximal unitigs of a canonical count table."""

from __future__ import annotations

from ctypes import byref, c_uint32, c_uint64, c_void_p
from dataclasses import dataclass
from typing import Optional

import numpy as np

from .. import _native as N
from .device import Device, DeviceBuffer
from .kmers import CountResult
from .output import _format
from .tables import _check_index_bits, _index, _index_bits


UNITIG_MIN_K, UNITIG_MAX_K = 3, 31


def check_unitig_k(k: int) -> int:
    """The K of the unitig graph, checked: odd (no k-mer is then its own
    reverse complement) and in [3, 31] (one 64-bit key, and a spare base)."""
    if isinstance(k, bool) or not isinstance(k, (int, np.integer)):
        raise AssertionError("K must be an integer, got %r" % (k,))
    if k > UNITIG_MAX_K:
        raise AssertionError("unitigs take K <= %d, got %d: larger K is a stated limit of this command"
                             % (UNITIG_MAX_K, k))
    if k < UNITIG_MIN_K:
        raise AssertionError("unitigs take K >= %d, got %d" % (UNITIG_MIN_K, k))
    if k % 2 == 0:
        raise AssertionError("unitigs take an odd K (a k-mer of even length can be its own reverse complement), "
                             "got %d" % k)
    return int(k)


@dataclass
class UnitigResult:
    """The unitigs of a table, on the host, in file order: unitig u is
    seqs[off[u]:off[u + 1]] (ASCII), made of nodes[u] rows whose counts sum to
    kc[u] (modulo 2^64).  rounds / cycles: what kman_graph_rank reports.
    eoff / edges (unitigs(.., links=True); else None): kman_unitig_edges' CSR,
    the edges of end e = 2 u + o are the words (v << 1) | p in
    edges[eoff[e]:eoff[e + 1]]."""
    seqs: np.ndarray
    off: np.ndarray
    nodes: np.ndarray
    kc: np.ndarray
    k: int
    rounds: int = 0
    cycles: int = 0
    eoff: Optional[np.ndarray] = None
    edges: Optional[np.ndarray] = None

    @property
    def n(self) -> int:
        return len(self.nodes)

    def seq(self, u: int) -> str:
        return self.seqs[int(self.off[u]):int(self.off[u + 1])].tobytes().decode()


def graph_links(dev: Device, table: CountResult, index: Optional[DeviceBuffer] = None,
                index_bits: Optional[int] = None) -> DeviceBuffer:
    """kman_graph_links: the 2 n link words of a canonical count table in a
    fresh device buffer.  `index` / `index_bits` as for screen."""
    k = check_unitig_k(table.k)
    bits = _index_bits(table, index_bits)
    with dev.scratch() as s:
        link = s.alloc(8 * max(table.n, 1))
        index = _index(s, table, index, bits)
        N.check(dev.ctx, N.lib().kman_graph_links(dev.ctx, c_void_p(table.ukeys.ptr), table.n, k, c_void_p(index.ptr),
                                                  bits, c_void_p(link.ptr)), "kman_graph_links")
        return s.keep(link)


def unitigs(dev: Device, table: CountResult, index: Optional[DeviceBuffer] = None,
            index_bits: Optional[int] = None, links: bool = False) -> UnitigResult:
    """The maximal unitigs of a CANONICAL count table (join_groups(..,
    "count", canonical=True), K odd and in [3, 31]) as include/kman.h defines
    them: kman_graph_links, kman_graph_rank, kman_unitig_spell (a sizing call,
    then the filling one), and one download.  `index`: a table_index(dev,
    table, index_bits) kept by the caller; None: built and freed here.  An
    empty table gives zero unitigs.  links=True: the edges between the unitigs
    too (kman_unitig_edges, one filling call into 8 U words, the most a graph
    of U unitigs has), with one index built here for both lookups."""
    k = check_unitig_k(table.k)
    n = int(table.n)
    if n >= N.KMAN_GRAPH_MAX_ROWS:
        raise AssertionError("unitigs take tables of fewer than 2^31 rows, got %d" % n)
    if n == 0:
        if index_bits is not None:
            _check_index_bits(index_bits, k)
        r = UnitigResult(np.zeros(0, np.uint8), np.zeros(1, np.uint64), np.zeros(0, np.uint32),
                         np.zeros(0, np.uint64), k)
        if links:
            r.eoff, r.edges = np.zeros(1, np.uint64), np.zeros(0, np.uint32)
        return r
    L = N.lib()
    with dev.scratch() as s:
        def alloc(nbytes):
            return s.alloc(max(16, nbytes))

        if links:
            bits = _index_bits(table, index_bits)
            index = _index(s, table, index, bits)  # (built once, for the links and for the edges)
        link = s.own(graph_links(dev, table, index, index_bits))
        rank = alloc(12 * n)
        start, pos, nodes = (c_void_p(rank.ptr + 4 * n * j) for j in range(3))
        rounds, cycles = c_uint32(0), c_uint64(0)
        N.check(dev.ctx, L.kman_graph_rank(dev.ctx, c_void_p(link.ptr), n, start, pos, nodes, byref(rounds),
                                           byref(cycles)), "kman_graph_rank")
        s.keep(link).free()  # (the links are done with before the spelling's buffers are made)
        nu, nb = c_uint64(0), c_uint64(0)
        keys, counts = c_void_p(table.ukeys.ptr), c_void_p(table.counts.ptr)
        N.check(dev.ctx, L.kman_unitig_spell(dev.ctx, keys, counts, table.count_bytes, n, k, start, pos, nodes, None,
                                             None, None, 0, None, 0, byref(nu), byref(nb)), "kman_unitig_spell")
        U, B = int(nu.value), int(nb.value)
        d_off, d_un, d_kc, d_seq = alloc(8 * (U + 1)), alloc(4 * U), alloc(8 * U), alloc(B)
        N.check(dev.ctx, L.kman_unitig_spell(dev.ctx, keys, counts, table.count_bytes, n, k, start, pos, nodes,
                                             c_void_p(d_off.ptr), c_void_p(d_un.ptr), c_void_p(d_kc.ptr), U,
                                             c_void_p(d_seq.ptr), B, byref(nu), byref(nb)), "kman_unitig_spell")
        assert int(nu.value) == U and int(nb.value) == B
        r = UnitigResult(dev.download(d_seq, B, np.uint8), dev.download(d_off, U + 1, np.uint64),
                         dev.download(d_un, U, np.uint32), dev.download(d_kc, U, np.uint64), k,
                         int(rounds.value), int(cycles.value))
        if links:
            d_eoff, d_edge = alloc(8 * (2 * U + 1)), alloc(4 * 8 * U)
            ne, ned = c_uint64(0), c_uint64(0)
            N.check(dev.ctx, L.kman_unitig_edges(dev.ctx, keys, n, k, c_void_p(index.ptr), bits, start, pos, nodes,
                                                 c_void_p(d_eoff.ptr), 2 * U, c_void_p(d_edge.ptr), 8 * U,
                                                 byref(ne), byref(ned)), "kman_unitig_edges")
            assert int(ne.value) == 2 * U and int(ned.value) <= 8 * U
            r.eoff = dev.download(d_eoff, 2 * U + 1, np.uint64)
            r.edges = dev.download(d_edge, int(ned.value), np.uint32)
        return r


_UNITIG_SLICE = 64 << 20  # bases formatted per call of the host writer
_GFA_LINK_SLICE = 4 << 20  # edges formatted per call of the host writer


def emit_unitigs(r: UnitigResult, sink=None):
    """The `kmer unitigs` text, ">ID LN:i:BASES KC:i:SUM" and the sequence on
    one line per unitig in file order (kman_format_unitigs on host threads, a
    slice of unitigs at a time).  Returned, or written to the binary file
    `sink`."""
    seqs = np.ascontiguousarray(r.seqs, dtype=np.uint8)
    off = np.ascontiguousarray(r.off, dtype=np.uint64)
    kc = np.ascontiguousarray(r.kc, dtype=np.uint64)
    n = len(kc)
    if len(off) != n + 1 or (n and int(off[n]) > len(seqs)):
        raise AssertionError("emit_unitigs: %d offsets and %d sequence bytes for %d unitigs" % (len(off), len(seqs), n))
    out, u0 = [], 0
    while u0 < n:
        u1 = int(np.searchsorted(off, int(off[u0]) + _UNITIG_SLICE, side="right")) - 1
        u1 = min(n, max(u1, u0 + 1))
        text = _format(N.lib().kman_format_unitigs, seqs.ctypes.data_as(c_void_p),
                       c_void_p(off.ctypes.data + 8 * u0), c_void_p(kc.ctypes.data + 8 * u0), u1 - u0, u0)
        if sink is None:
            out.append(text)
        else:
            sink.write(text)
        u0 = u1
    return b"".join(out) if sink is None else None


def emit_gfa(r: UnitigResult, sink=None):
    """The `kmer unitigs --gfa` text, GFA 1.0: "H\tVN:Z:1.0", then one
    "S\tID\tSEQ\tLN:i:BASES\tKC:i:SUM" line per unitig, then one
    "L\tU\t+|-\tV\t+|-\t(K-1)M" line per edge in the order of r.eoff
    (kman_format_gfa_segments and kman_format_gfa_links on host threads, a
    slice of unitigs at a time, as emit_unitigs).  r: a result of unitigs(..,
    links=True).  Returned, or written to the binary file `sink`."""
    if r.eoff is None or r.edges is None:
        raise AssertionError("emit_gfa: the result holds no links (unitigs(.., links=True) makes them)")
    seqs = np.ascontiguousarray(r.seqs, dtype=np.uint8)
    off = np.ascontiguousarray(r.off, dtype=np.uint64)
    kc = np.ascontiguousarray(r.kc, dtype=np.uint64)
    eoff = np.ascontiguousarray(r.eoff, dtype=np.uint64)
    edges = np.ascontiguousarray(r.edges, dtype=np.uint32)
    n = len(kc)
    if len(off) != n + 1 or (n and int(off[n]) > len(seqs)):
        raise AssertionError("emit_gfa: %d offsets and %d sequence bytes for %d unitigs" % (len(off), len(seqs), n))
    if len(eoff) != 2 * n + 1 or int(eoff[2 * n]) - int(eoff[0]) > len(edges):
        raise AssertionError("emit_gfa: %d end offsets and %d edges for %d unitigs" % (len(eoff), len(edges), n))
    if len(edges) and int(edges.max()) >> 1 >= n:
        raise AssertionError("emit_gfa: an edge names unitig %d of %d" % (int(edges.max()) >> 1, n))
    out = []

    def put(text):
        if sink is None:
            out.append(text)
        else:
            sink.write(text)

    put(b"H\tVN:Z:1.0\n")
    u0 = 0
    while u0 < n:
        u1 = int(np.searchsorted(off, int(off[u0]) + _UNITIG_SLICE, side="right")) - 1
        u1 = min(n, max(u1, u0 + 1))
        put(_format(N.lib().kman_format_gfa_segments, seqs.ctypes.data_as(c_void_p),
                    c_void_p(off.ctypes.data + 8 * u0), c_void_p(kc.ctypes.data + 8 * u0), u1 - u0, u0))
        u0 = u1
    u0, e0 = 0, int(eoff[0]) if n else 0
    while u0 < n:
        u1 = (int(np.searchsorted(eoff, int(eoff[2 * u0]) + _GFA_LINK_SLICE, side="right")) - 1) // 2
        u1 = min(n, max(u1, u0 + 1))
        put(_format(N.lib().kman_format_gfa_links, c_void_p(eoff.ctypes.data + 16 * u0),
                    c_void_p(edges.ctypes.data + 4 * (int(eoff[2 * u0]) - e0)), u1 - u0, u0, r.k))
        u0 = u1
    return b"".join(out) if sink is None else None
