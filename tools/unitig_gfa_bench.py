#!/usr/bin/env python3
"""Time the edges pass of `kmer unitigs --gfa` (HIP events of kman_timing, tag
"unitig_edges") next to "graph_links" on the same table in the same run, on
the two tables of tools/unitig_bench.py at K = 31 (its genome and its reads):
1 warm-up + 2 timed runs of engine.unitigs(links=True), then the same of
engine.unitigs() without links, whose four tags are what `kmer unitigs`
without --gfa costs."""
import argparse
import ctypes
import os
import sys
import time
from ctypes import byref, c_uint64

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np  # noqa: E402

import unitig_bench as ub  # noqa: E402
from kman_amd import _native as N  # noqa: E402
from kman_amd import engine  # noqa: E402

TAGS = ub.TAGS + (b"unitig_edges",)


def timed(dev, table, links: bool):
    L = N.lib()
    for _ in range(ub.WARM):
        r = engine.unitigs(dev, table, links=links)
    L.kman_timing_enable(dev.ctx, 1)
    t0 = time.perf_counter()
    for _ in range(ub.TIMED):
        r = engine.unitigs(dev, table, links=links)
    wall = (time.perf_counter() - t0) / ub.TIMED
    ms = {}
    for tag in TAGS:
        cnt, t = c_uint64(), ctypes.c_double()
        L.kman_timing_query(dev.ctx, tag, byref(cnt), byref(t))
        ms[tag.decode()] = t.value / ub.TIMED
    L.kman_timing_enable(dev.ctx, 0)
    return r, ms, wall


def run(dev, name: str, table) -> list:
    n = int(table.n)
    r, ms, wall = timed(dev, table, True)
    per_end = np.bincount(np.diff(r.eoff.astype(np.int64)), minlength=5)
    assert len(r.eoff) == 2 * r.n + 1 and int(r.eoff[-1]) == len(r.edges) and per_end[5:].sum() == 0
    assert len(r.edges) == 0 or int(r.edges.max()) >> 1 < r.n
    # every edge (e, w) has its mirror (w ^ 1, e ^ 1), and none occurs twice
    e = np.repeat(np.arange(2 * r.n, dtype=np.uint64), np.diff(r.eoff.astype(np.int64)))
    w = r.edges.astype(np.uint64)
    fwd, back = np.sort((e << np.uint64(32)) | w), np.sort(((w ^ np.uint64(1)) << np.uint64(32)) | (e ^ np.uint64(1)))
    assert np.array_equal(fwd, back) and (len(fwd) < 2 or np.all(fwd[1:] != fwd[:-1]))
    _, plain, plain_wall = timed(dev, table, False)
    return [
        "%s: %d rows, U = %d unitigs, E = %d edges (ends with 0..4 edges: %s), index bits %d"
        % (name, n, r.n, len(r.edges), " ".join(str(int(c)) for c in per_end[:5]), engine.default_index_bits(n, ub.K)),
        "%s --gfa: unitig_edges %.3f ms next to graph_links %.3f ms (ratio %.2f); table_index %.3f ms, graph_rank "
        "%.3f ms, unitig_spell %.3f ms; engine.unitigs(links=True) %.1f ms wall with its downloads"
        % (name, ms["unitig_edges"], ms["graph_links"], ms["unitig_edges"] / max(1e-9, ms["graph_links"]),
           ms["table_index"], ms["graph_rank"], ms["unitig_spell"], 1e3 * wall),
        "%s without --gfa: table_index %.3f ms, graph_links %.3f ms, graph_rank %.3f ms, unitig_spell %.3f ms, "
        "unitig_edges %.3f ms; kernels %.3f ms; engine.unitigs %.1f ms wall"
        % (name, plain["table_index"], plain["graph_links"], plain["graph_rank"], plain["unitig_spell"],
           plain["unitig_edges"], sum(plain.values()), 1e3 * plain_wall),
    ]


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--bases", type=int, default=200_000_000)
    ap.add_argument("--read-bases", type=int, default=20_000_000)
    ap.add_argument("--coverage", type=float, default=5.0)
    ap.add_argument("--error", type=float, default=0.01)
    ap.add_argument("--out", default=None, help="also append the lines to this file")
    a = ap.parse_args()
    rng = np.random.default_rng(2024)
    genome = rng.integers(0, 4, a.bases, dtype=np.uint8)
    dev = engine.Device(0)
    lines = ["K = %d, %d + %d runs, genome %d bases in records of %d, reads of %d bases at %.1fx of the first %d "
             "bases, error %.3f" % (ub.K, ub.WARM, ub.TIMED, a.bases, ub.REC, ub.READ, a.coverage,
                                    min(a.read_bases, a.bases), a.error)]
    t = ub.table_of(dev, ub.fasta_of(genome, ub.REC, "g"))
    lines += run(dev, "genome", t)
    engine.free_result(t)
    print("\n".join(lines), flush=True)
    reads = ub.reads_of(genome[:a.read_bases], a.coverage, a.error, rng)
    t = ub.table_of(dev, ub.fasta_of(reads.reshape(-1), ub.READ, "r"))
    del reads
    lines += run(dev, "reads -L 1", t)
    engine.free_result(t)
    dev.close()
    print("\n".join(lines[4:]), flush=True)
    if a.out:
        with open(a.out, "a") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
