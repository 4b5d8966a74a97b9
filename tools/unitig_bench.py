#!/usr/bin/env python3
"""Time the kernels behind `kmer unitigs` (HIP events of kman_timing around
their launches, tags "table_index", "graph_links", "graph_rank" and
"unitig_spell"; 1 warm-up + 2 timed runs of engine.unitigs, downloads aside)
on two tables at K = 31:

  genome  --bases bases (default 200 M) of uniform random sequence in records
          of 1 Mbp: nearly every k-mer has one neighbour on each side, a few
          long unitigs per record;
  reads   150-base reads drawn from the first --read-bases bases of it at
          --coverage, both strands, each base replaced with probability
          --error: every error forks the graph, many short unitigs (-L 1).

Beside the GPU numbers, for scale: the plain-Python statement of
tests/unitig_cases.py on the first 1 Mbp of the genome, timed on the host, and
its unitigs compared with the GPU's for equality."""
import argparse
import ctypes
import os
import sys
import time
from ctypes import byref, c_uint64

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402

import unitig_cases as uc  # noqa: E402
from kman_amd import _native as N  # noqa: E402
from kman_amd import engine  # noqa: E402

K = 31
WARM, TIMED = 1, 2
REC = 1_000_000
READ = 150
TAGS = (b"table_index", b"graph_links", b"graph_rank", b"unitig_spell")
_ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)


def fasta_of(codes: np.ndarray, rec: int, prefix: str) -> bytes:
    """One line per record of `rec` bases."""
    parts = []
    for r, lo in enumerate(range(0, len(codes), rec)):
        parts.append(b">%s%d\n" % (prefix.encode(), r))
        parts.append(_ACGT[codes[lo:lo + rec]].tobytes())
        parts.append(b"\n")
    return b"".join(parts)


def reads_of(genome: np.ndarray, coverage: float, error: float, rng) -> np.ndarray:
    """(n_reads, READ) codes: windows of the genome, half of them reverse
    complemented, with substitution errors."""
    n = int(len(genome) * coverage / READ)
    starts = rng.integers(0, len(genome) - READ, n)
    r = genome[starts[:, None] + np.arange(READ)[None, :]]
    flip = rng.random(n) < 0.5
    r[flip] = (3 - r[flip])[:, ::-1]
    err = rng.random(r.shape) < error
    r[err] = (r[err] + rng.integers(1, 4, int(err.sum())).astype(np.uint8)) & 3
    return r


def table_of(dev, text: bytes):
    p = engine.parse(dev, text)
    try:
        return engine.join_groups(p, K, False, "count", canonical=True)
    finally:
        p.free()


def run(dev, name: str, table) -> list:
    L = N.lib()
    for _ in range(WARM):
        r = engine.unitigs(dev, table)
    L.kman_timing_enable(dev.ctx, 1)
    t0 = time.perf_counter()
    for _ in range(TIMED):
        r = engine.unitigs(dev, table)
    wall = (time.perf_counter() - t0) / TIMED
    ms = {}
    for tag in TAGS:
        cnt, t = c_uint64(), ctypes.c_double()
        L.kman_timing_query(dev.ctx, tag, byref(cnt), byref(t))
        ms[tag.decode()] = t.value / TIMED
    L.kman_timing_enable(dev.ctx, 0)
    n = int(table.n)
    lens = np.diff(r.off.astype(np.int64))
    order = np.sort(lens)[::-1]
    n50 = int(order[np.searchsorted(np.cumsum(order), lens.sum() / 2)]) if len(lens) else 0
    assert int(r.nodes.sum()) == n and int(lens.sum()) == n + r.n * (K - 1)
    kern = sum(ms.values())
    return [
        "%s: %d rows, %d unitigs (longest %d, N50 %d bases), %d rounds that moved, %d cycles cut, index bits %d"
        % (name, n, r.n, int(lens.max()) if len(lens) else 0, n50, r.rounds, r.cycles,
           engine.default_index_bits(n, K)),
        "%s: table_index %.3f ms, graph_links %.3f ms, graph_rank %.3f ms (%.3f ms per launched round), "
        "unitig_spell %.3f ms; kernels %.3f ms = %.2f ns per row; engine.unitigs %.1f ms wall with its downloads"
        % (name, ms["table_index"], ms["graph_links"], ms["graph_rank"], ms["graph_rank"] / max(1, r.rounds + 1),
           ms["unitig_spell"], kern, 1e6 * kern / max(1, n), 1e3 * wall),
    ]


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--bases", type=int, default=200_000_000)
    ap.add_argument("--read-bases", type=int, default=20_000_000)
    ap.add_argument("--coverage", type=float, default=5.0)
    ap.add_argument("--error", type=float, default=0.01)
    ap.add_argument("--slice", type=int, default=1_000_000, help="bases of the host statement's run")
    ap.add_argument("--out", default=None, help="also append the lines to this file")
    a = ap.parse_args()
    rng = np.random.default_rng(2024)
    genome = rng.integers(0, 4, a.bases, dtype=np.uint8)
    dev = engine.Device(0)
    lines = ["K = %d, %d + %d runs, genome %d bases in records of %d, reads of %d bases at %.1fx of the first %d "
             "bases, error %.3f" % (K, WARM, TIMED, a.bases, REC, READ, a.coverage, min(a.read_bases, a.bases),
                                    a.error)]
    t = table_of(dev, fasta_of(genome, REC, "g"))
    lines += run(dev, "genome", t)
    engine.free_result(t)
    reads = reads_of(genome[:a.read_bases], a.coverage, a.error, rng)
    t = table_of(dev, fasta_of(reads.reshape(-1), READ, "r"))
    del reads
    lines += run(dev, "reads -L 1", t)
    engine.free_result(t)
    # the statement on a slice, on the host
    piece = _ACGT[genome[:a.slice]].tobytes().decode()
    t0 = time.perf_counter()
    want = uc.unitigs(uc.table_of([("s", piece)], K))
    host_s = time.perf_counter() - t0
    t = table_of(dev, b">s\n" + piece.encode() + b"\n")
    L = N.lib()
    L.kman_timing_enable(dev.ctx, 1)
    r = engine.unitigs(dev, t)
    gpu_ms = 0.0
    for tag in TAGS:
        cnt, ms = c_uint64(), ctypes.c_double()
        L.kman_timing_query(dev.ctx, tag, byref(cnt), byref(ms))
        gpu_ms += ms.value
    L.kman_timing_enable(dev.ctx, 0)
    got = [(r.seq(u), int(r.nodes[u]), int(r.kc[u])) for u in range(r.n)]
    assert got == want, "the GPU's unitigs of the slice differ from the statement's"
    lines.append("slice of %d bases: %d rows, %d unitigs, equal to the host statement's; the statement (plain Python, one "
                 "thread) %.1f s, the GPU kernels %.3f ms (first run, not warmed)"
                 % (a.slice, int(t.n), r.n, host_s, gpu_ms))
    engine.free_result(t)
    dev.close()
    print("\n".join(lines), flush=True)
    if a.out:
        with open(a.out, "a") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
