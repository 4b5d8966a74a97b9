"""`kmer compare` test helper (not a conftest): a plain-Python statement of
kman_mask_gram, engine.compare_rows and the command's OUTPUT, --matrix,
--occupancy and --summary files (include/kman.h, `kmer compare --help`),
independent of the code under test.  It builds on tests/classify_cases.py (the
coloured table of some references) and tests/screen_cases.py (records,
windows, tables).

An input is a list of ``(name, sequence)`` records; input c is bit c of a
k-mer's mask.
"""

from __future__ import annotations

import math
from collections import Counter

import numpy as np

import classify_cases as cc
import screen_cases as sc

METRICS = ("jaccard", "dist", "shared", "containment")


def mask_gram(masks, n_colors: int):
    """kman_mask_gram of a sequence of masks: (G, occ, private) as lists of
    Python ints, G of n_colors rows.  Loops over the rows and the pairs of set
    bits of each; equal masks are taken together (a row count, not another
    rule)."""
    cut = (1 << n_colors) - 1
    G = [[0] * n_colors for _ in range(n_colors)]
    occ = [0] * (n_colors + 1)
    private = [0] * n_colors
    for m, rows in Counter(int(x) & cut for x in masks).items():
        bits = [c for c in range(n_colors) if (m >> c) & 1]
        occ[len(bits)] += rows
        if len(bits) == 1:
            private[bits[0]] += rows
        for i in bits:
            for j in bits:
                G[i][j] += rows
    return G, occ, private


def as_arrays(G, occ, private):
    nc = len(G)
    return (np.asarray(G, dtype=np.uint64).reshape(nc, nc), np.asarray(occ, dtype=np.uint64),
            np.asarray(private, dtype=np.uint64))


def metrics(a: int, b: int, s: int, k: int):
    """(jaccard, containment of the first, of the second, Mash distance)."""
    u = a + b - s
    jac = s / u if u else 0.0
    ca = s / a if a else 0.0
    cb = s / b if b else 0.0
    if jac == 0.0:
        dist = 1.0
    elif jac == 1.0:
        dist = 0.0
    else:
        dist = min(1.0, max(0.0, -math.log(2.0 * jac / (1.0 + jac)) / k))
    return jac, ca, cb, dist


def rows(G, k: int):
    """(i, j, a, b, s, jaccard, cont_i, cont_j, dist) per pair i < j."""
    out = []
    for i in range(len(G)):
        for j in range(i + 1, len(G)):
            a, b, s = int(G[i][i]), int(G[j][j]), int(G[i][j])
            out.append((i, j, a, b, s) + metrics(a, b, s, k))
    return out


def lines(labels, G, k: int) -> bytes:
    return "".join("%s\t%s\t%d\t%d\t%d\t%.6f\t%.6f\t%.6f\t%.6f\n" % ((labels[r[0]], labels[r[1]]) + r[2:])
                   for r in rows(G, k)).encode()


def matrix(labels, G, k: int, metric: str = "dist") -> bytes:
    n = len(G)
    out = ["%d\n" % n]
    for r in range(n):
        cells = []
        for c in range(n):
            a, b, s = int(G[r][r]), int(G[c][c]), int(G[r][c])
            jac, ca, _, dist = metrics(a, b, s, k)
            if r == c:
                jac = ca = 1.0 if a else 0.0
                dist = 0.0
            cells.append({"shared": "%d" % s, "jaccard": "%.6f" % jac, "containment": "%.6f" % ca,
                          "dist": "%.6f" % dist}[metric])
        out.append("\t".join([labels[r]] + cells) + "\n")
    return "".join(out).encode()


def occupancy(occ) -> bytes:
    return "".join("%d\t%d\n" % (p, int(occ[p])) for p in range(1, len(occ))).encode()


def summary(labels, G, private) -> bytes:
    return "".join("%s\t%d\t%d\n" % (lab, int(G[c][c]), int(private[c])) for c, lab in enumerate(labels)).encode()


def compare(inputs, k: int, canonical: bool = False, min_count: int = 1, max_count=None):
    """The whole command on inputs (lists of records): (G, occ, private)."""
    ct = cc.color_table_of(inputs, k, canonical, min_count, max_count)
    return mask_gram(ct.values(), len(inputs))


# ------------------------------------------------------------------ builders


def planted_inputs(seed: int = 1, length: int = 300):
    """Three random inputs of a few hundred bases with planted shared
    segments (one held by all three, one by the first two, one by the last
    two, the second also twice in the second input), and one empty input."""
    rng = np.random.default_rng(seed)
    core, ab, bc = sc.rand_seq(rng, 70), sc.rand_seq(rng, 60), sc.rand_seq(rng, 50)
    a = [("a0", sc.rand_seq(rng, length) + core), ("a1", ab + sc.rand_seq(rng, 40))]
    b = [("b0", core + sc.rand_seq(rng, length // 2) + ab), ("b1", bc), ("b2", "N" + ab)]
    c = [("c0", sc.rand_seq(rng, length) + "N" + bc + core)]
    return [a, b, c, []]


def mask_cases(n: int, n_colors: int, seed: int) -> dict:
    """name -> n u64 masks: all ones, all zero, one bit each round-robin,
    random dense, random sparse, and random with garbage in the bits at or
    above n_colors."""
    rng = np.random.default_rng(seed)
    cut = np.uint64((1 << n_colors) - 1)
    dense = rng.integers(0, 1 << 64, n, dtype=np.uint64)
    sparse = dense & rng.integers(0, 1 << 64, n, dtype=np.uint64) & rng.integers(0, 1 << 64, n, dtype=np.uint64) \
        & rng.integers(0, 1 << 64, n, dtype=np.uint64)
    return {
        "ones": np.full(n, (1 << 64) - 1, dtype=np.uint64) & cut,
        "zero": np.zeros(n, dtype=np.uint64),
        "one_bit": np.asarray([1 << (r % n_colors) for r in range(n)], dtype=np.uint64),
        "dense": dense & cut,
        "sparse": sparse & cut,
        "garbage": dense | ~cut,  # (every bit at or above n_colors is set)
    }
