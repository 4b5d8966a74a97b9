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
    kc[u] (modulo 2^64).  rounds / cycles: what kman_graph_rank reports."""
    seqs: np.ndarray
    off: np.ndarray
    nodes: np.ndarray
    kc: np.ndarray
    k: int
    rounds: int = 0
    cycles: int = 0

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
            index_bits: Optional[int] = None) -> UnitigResult:
    """The maximal unitigs of a CANONICAL count table (join_groups(..,
    "count", canonical=True), K odd and in [3, 31]) as include/kman.h defines
    them: kman_graph_links, kman_graph_rank, kman_unitig_spell (a sizing call,
    then the filling one), and one download.  `index`: a table_index(dev,
    table, index_bits) kept by the caller; None: built and freed here.  An
    empty table gives zero unitigs."""
    k = check_unitig_k(table.k)
    n = int(table.n)
    if n >= N.KMAN_GRAPH_MAX_ROWS:
        raise AssertionError("unitigs take tables of fewer than 2^31 rows, got %d" % n)
    if n == 0:
        if index_bits is not None:
            _check_index_bits(index_bits, k)
        return UnitigResult(np.zeros(0, np.uint8), np.zeros(1, np.uint64), np.zeros(0, np.uint32),
                            np.zeros(0, np.uint64), k)
    L = N.lib()
    with dev.scratch() as s:
        def alloc(nbytes):
            return s.alloc(max(16, nbytes))

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
        return UnitigResult(dev.download(d_seq, B, np.uint8), dev.download(d_off, U + 1, np.uint64),
                            dev.download(d_un, U, np.uint32), dev.download(d_kc, U, np.uint64), k,
                            int(rounds.value), int(cycles.value))


_UNITIG_SLICE = 64 << 20  # bases formatted per call of the host writer


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
