"""`kmer unitigs --gfa` test helper (not a conftest): the plain-Python statement
of the edges between unitigs as include/kman.h defines them, once on the
unitig texts and once on the table's rows, the CSR form kman_unitig_edges
writes, the GFA text, a GFA parser, and cases at the edges of the kernel's
tiles.

An edge is (u, o, v, p): unitig u in orientation o (0 = "+", its text; 1 =
"-", the reverse complement) is followed by unitig v in orientation p.  End
e = 2 u + o is the right end of the oriented text.
"""

from __future__ import annotations

import numpy as np

import screen_cases as sc
import unitig_cases as uc

R, L = uc.R, uc.L


def oriented(s: str, o: int) -> str:
    return s if o == 0 else sc.revcomp(s)


def edges_text(units, k: int):
    """[(u, o, v, p)] from the texts alone: ends in the order of e, within an
    end the bases A, C, G, T that extend the oriented text."""
    first = {}
    for v, s in enumerate(units):
        for p in (0, 1):
            w = oriented(s, p)[:k]
            assert w not in first, "two oriented unitigs begin with %s" % w
            first[w] = (v, p)
    out = []
    for u, s in enumerate(units):
        for o in (0, 1):
            tail = oriented(s, o)[-(k - 1):]
            for b in "ACGT":
                if tail + b in first:
                    out.append((u, o) + first[tail + b])
    return out


def edges_rows(table: dict):
    """The same list from the rows: the walks of unitig_cases and the
    neighbours of the header's definition."""
    kmers, row = uc.rows_of(table)
    walks = uc.walks(table)[0]
    plus, minus = {}, {}
    for v, walk in enumerate(walks):
        (j0, s0), (j1, s1) = walk[0], walk[-1]
        plus[(j0, s0 ^ 1)] = v  # entered at the side opposite the one the first row is left through
        minus[(j1, s1)] = v  # entered at the side the last row is left through
    out = []
    for u, walk in enumerate(walks):
        (j0, s0), (j1, s1) = walk[0], walk[-1]
        for o, (i, s) in enumerate(((j1, s1), (j0, s0 ^ 1))):
            nb = uc.neighbours(kmers[i], s, row)
            if s == L:
                nb = nb[::-1]  # b + x[:-1] read on the other strand: the extension is the complement of b
            for jt in nb:
                assert (jt in plus) != (jt in minus), "a neighbour of an end names exactly one oriented unitig"
                out.append((u, o, plus[jt], 0) if jt in plus else (u, o, minus[jt], 1))
    return out


def csr(edges, U: int):
    """(eoff of 2 U + 1 u64, edge of E u32) as kman_unitig_edges writes them."""
    eoff = np.zeros(2 * U + 1, dtype=np.uint64)
    for u, o, _, _ in edges:
        eoff[2 * u + o + 1] += 1
    eoff = np.cumsum(eoff).astype(np.uint64)
    assert [2 * u + o for u, o, _, _ in edges] == sorted(2 * u + o for u, o, _, _ in edges)
    return eoff, np.asarray([(v << 1) | p for _, _, v, p in edges], dtype=np.uint32)


def uncsr(eoff, edge):
    out = []
    for e in range(len(eoff) - 1):
        for w in edge[int(eoff[e]):int(eoff[e + 1])]:
            out.append((e >> 1, e & 1, int(w) >> 1, int(w) & 1))
    return out


def segments_text(units, first_id: int = 0) -> bytes:
    """units: [(sequence, rows, KC)] as unitig_cases.unitigs gives them."""
    return "".join("S\t%d\t%s\tLN:i:%d\tKC:i:%d\n" % (first_id + u, s, len(s), kc)
                   for u, (s, _, kc) in enumerate(units)).encode()


def links_text(edges, k: int) -> bytes:
    return "".join("L\t%d\t%s\t%d\t%s\t%dM\n" % (u, "+-"[o], v, "+-"[p], k - 1) for u, o, v, p in edges).encode()


def gfa_text(units, edges, k: int) -> bytes:
    return b"H\tVN:Z:1.0\n" + segments_text(units) + links_text(edges, k)


def parse_gfa(data: bytes):
    """(units as [(sequence, KC)], edges, the overlap of every L line) of a
    GFA 1.0 file written by `kmer unitigs --gfa`: the header first, then every
    S line, then every L line."""
    lines = data.decode().split("\n")
    assert lines[0] == "H\tVN:Z:1.0" and lines[-1] == ""
    units, edges, overlaps = [], [], set()
    for line in lines[1:-1]:
        f = line.split("\t")
        if f[0] == "S":
            assert not edges and int(f[1]) == len(units) and f[3] == "LN:i:%d" % len(f[2]) and f[4].startswith("KC:i:")
            units.append((f[2], int(f[4][5:])))
        else:
            assert f[0] == "L" and len(f) == 6 and f[2] in "+-" and f[4] in "+-" and f[5].endswith("M")
            edges.append((int(f[1]), "+-".index(f[2]), int(f[3]), "+-".index(f[4])))
            overlaps.add(int(f[5][:-1]))
    return units, edges, overlaps


def table_edges(table: dict, k: int):
    """(units, edges) of a table, both formulations held equal."""
    units = uc.unitigs(table)
    edges = edges_text([s for s, _, _ in units], k)
    assert edges == edges_rows(table)
    return units, edges


# ------------------------------------------------------------- tile edges


def tile_case(n_units: int, seed: int, k: int = 21):
    """Records whose table has exactly n_units unitigs in disjoint components:
    about one in eight a y_fork (3 unitigs, 4 edges) or a fork_and_merge (5
    unitigs, 8 edges) of fresh random paths, the rest single paths of 1..3
    rows without an edge.  The caller asserts U with the statement."""
    records, left, c = [], n_units, 0
    while left:
        s0 = seed * 100000 + 10 * c
        kind = c % 16
        if kind == 3 and left >= 3:
            stem, a, b = (uc.path_seq(n, k, s0 + j) for j, n in enumerate((4, 3, 5)))
            records += [("f%da" % c, stem + a), ("f%db" % c, stem + b)]
            left -= 3
        elif kind == 11 and left >= 5:
            a, stem, b, x, y = (uc.path_seq(n, k, s0 + j) for j, n in enumerate((3, 4, 2, 2, 3)))
            records += [("m%dx" % c, a + stem + b), ("m%dy" % c, x + stem + y)]
            left -= 5
        else:
            records.append(("p%d" % c, uc.path_seq(1 + c % 3, k, s0)))
            left -= 1
        c += 1
    return records, k, 1


def tile_cases(tile: int) -> dict:
    """2 U at tile - 2, tile, tile + 2 and 3 tile + 2 ends."""
    return {"ends_%d" % n2: tile_case(n2 // 2, 7 + i)
            for i, n2 in enumerate((tile - 2, tile, tile + 2, 3 * tile + 2))}
