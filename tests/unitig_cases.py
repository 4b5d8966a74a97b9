"""`kmer unitigs` test helper (not a conftest): a plain-Python statement of the
unitig definition of include/kman.h, dict-based and written from that text
alone, two order-free checkers, and the named cases.

A table is a dict canonical k-mer -> count; row i is the i-th k-mer in str
order (A < C < G < T is also the order of the 2-bit keys).  Sides: R = 0, L =
1; a (row, side) pair packs as (row << 1) | side.
"""

from __future__ import annotations

import numpy as np

import screen_cases as sc

R, L = 0, 1
NONE = 0xFFFFFFFF
MASK64 = (1 << 64) - 1


def canon(s: str) -> str:
    r = sc.revcomp(s)
    return s if s < r else r


def rows_of(table: dict):
    """(the k-mers in row order, k-mer -> row)."""
    kmers = sorted(table)
    return kmers, {w: i for i, w in enumerate(kmers)}


def neighbours(x: str, side: int, row: dict):
    """The (row, side entered) of every base that gives a neighbour, with
    repeats: deg is the length."""
    out = []
    for b in "ACGT":
        y = x[1:] + b if side == R else b + x[:-1]
        c = canon(y)
        if c in row:
            if side == R:
                out.append((row[c], L if y == c else R))
            else:
                out.append((row[c], R if y == c else L))
    return out


def links(table: dict) -> dict:
    """(i, s) -> (j, t) for every linked side."""
    kmers, row = rows_of(table)
    nb = {(i, s): neighbours(x, s, row) for i, x in enumerate(kmers) for s in (R, L)}
    out = {}
    for (i, s), v in nb.items():
        if len(v) == 1 and len(nb[v[0]]) == 1 and v[0][0] != i:
            out[(i, s)] = v[0]
    return out


def link_array(table: dict) -> np.ndarray:
    """kman_graph_links' d_link: 2 n u32 words."""
    out = np.full(2 * len(table), NONE, dtype=np.uint32)
    for (i, s), (j, t) in links(table).items():
        out[2 * i + s] = (j << 1) | t
    return out


def _cut_cycles(table: dict, link: dict) -> int:
    """Removes, for every cycle, the link at side L of its smallest row and
    its partner; returns the number of cycles."""
    seen, cycles = set(), 0
    for i in range(len(table)):
        if i in seen:
            continue
        nodes, cur, cyc = [i], (i, R), False
        while cur in link:
            j, t = link[cur]
            if j == i:
                cyc = True
                break
            nodes.append(j)
            cur = (j, t ^ 1)
        if not cyc:
            cur = (i, L)
            while cur in link:
                j, t = link[cur]
                nodes.append(j)
                cur = (j, t ^ 1)
        seen.update(nodes)
        if cyc:
            m = min(nodes)
            p = link.pop((m, L))
            link.pop(p)
            cycles += 1
    return cycles


def walks(table: dict):
    """The unitigs in file order as lists of (row, orientation): 0 = the row
    is left through R (spelled as it is), 1 = through L (reverse complement);
    and the number of cycles that were cut."""
    link = links(table)
    cycles = _cut_cycles(table, link)
    seen, out = set(), []
    for i in range(len(table)):
        if i in seen or ((i, R) in link and (i, L) in link):
            continue  # (an inner row; an end row that was already walked to is the larger end)
        s = L if (i, L) in link else R  # (a lone row is left through R)
        walk, cur = [(i, s)], (i, s)
        while cur in link:
            j, t = link[cur]
            cur = (j, t ^ 1)
            walk.append(cur)
        assert walk[-1][0] >= i  # the start is the smaller end
        seen.update(j for j, _ in walk)
        out.append(walk)
    assert len(seen) == len(table)
    return out, cycles


def unitigs(table: dict):
    """[(sequence, rows, KC)] in file order."""
    kmers, _ = rows_of(table)
    out = []
    for walk in walks(table)[0]:
        spelled = [kmers[j] if s == R else sc.revcomp(kmers[j]) for j, s in walk]
        seq = spelled[0] + "".join(w[-1] for w in spelled[1:])
        out.append((seq, len(walk), sum(table[kmers[j]] for j, _ in walk) & MASK64))
    return out


def rank_arrays(table: dict):
    """kman_graph_rank's (d_start, d_pos, d_nodes)."""
    n = len(table)
    start, pos, nodes = (np.zeros(n, dtype=np.uint32) for _ in range(3))
    for walk in walks(table)[0]:
        for p, (j, s) in enumerate(walk):
            start[j], pos[j] = walk[0][0], (p << 1) | s
        nodes[walk[0][0]] = len(walk)
    return start, pos, nodes


def text(units, first_id: int = 0) -> bytes:
    return "".join(">%d LN:i:%d KC:i:%d\n%s\n" % (first_id + u, len(s), kc, s)
                   for u, (s, _, kc) in enumerate(units)).encode()


def parse_text(data: bytes, k: int):
    """The (sequence, rows, KC) of a `kmer unitigs` file; checks ID and LN."""
    lines = data.decode().split("\n")
    assert lines[-1] == "" and len(lines) % 2 == 1
    out = []
    for u in range(len(lines) // 2):
        head, seq = lines[2 * u], lines[2 * u + 1]
        name, ln, kc = head.split(" ")
        assert name == ">%d" % u and ln == "LN:i:%d" % len(seq) and kc.startswith("KC:i:")
        out.append((seq, len(seq) - k + 1, int(kc[5:])))
    return out


# ------------------------------------------------------------------ checkers


def check_cover(seqs, table: dict, k: int) -> None:
    """(a): the canonical k-mers of all unitigs are the table's rows, each
    exactly once."""
    seen = {}
    for s in seqs:
        assert len(s) >= k
        for i in range(len(s) - k + 1):
            c = canon(s[i:i + k])
            seen[c] = seen.get(c, 0) + 1
    assert set(seen) == set(table)
    assert all(v == 1 for v in seen.values())


def _sides(w: str, row: dict):
    """(row, side the spelled k-mer w is left through to its right)."""
    c = canon(w)
    return row[c], R if w == c else L


def check_maximal(seqs, table: dict, k: int) -> None:
    """(b): every junction inside a unitig is a link, and no link joins the
    end of one unitig to the end of another (a link between a unitig's own two
    ends is a cycle that was cut)."""
    _, row = rows_of(table)
    link = links(table)
    for s in seqs:
        ws = [s[i:i + k] for i in range(len(s) - k + 1)]
        for a, b in zip(ws, ws[1:]):
            i, si = _sides(a, row)
            j, sj = _sides(b, row)
            assert link.get((i, si)) == (j, sj ^ 1)
        i, si = _sides(ws[0], row)
        j, sj = _sides(ws[-1], row)
        first_end, last_end = (i, si ^ 1), (j, sj)
        assert link.get(first_end) in (None, last_end)
        assert link.get(last_end) in (None, first_end)
        if len(ws) == 1:
            assert first_end not in link and last_end not in link  # (a row never links to itself)


# -------------------------------------------------------------------- cases


def table_of(records, k: int, min_count: int = 1, max_count=None) -> dict:
    return sc.table_of(records, k, True, min_count, max_count)


def path_seq(nodes: int, k: int, seed: int) -> str:
    """A random sequence of nodes + k - 1 bases that the statement spells as
    one unitig (no k-mer twice, no branch): checked, not assumed."""
    rng = np.random.default_rng(seed)
    for _ in range(100):
        s = sc.rand_seq(rng, nodes + k - 1)
        units = unitigs(table_of([("s", s)], k))
        if len(units) == 1 and units[0][1] == nodes:
            return s
    raise AssertionError("no repeat-free sequence of %d nodes at k = %d" % (nodes, k))


def cycle_seq(nodes: int, k: int, seed: int) -> str:
    """A circle of `nodes` bases that is one cyclic unitig of as many rows, as
    the linear text that holds every k-mer of the circle (the circle repeated
    until k - 1 bases past one turn): checked with the statement."""
    rng = np.random.default_rng(seed)
    for _ in range(1000):
        s = sc.rand_seq(rng, nodes)
        lin = (s * (1 + (k - 1 + nodes - 1) // nodes + 1))[:nodes + k - 1]
        t = table_of([("s", lin)], k)
        w, cycles = walks(t)
        if len(t) == nodes and len(w) == 1 and cycles == 1:
            return lin
    raise AssertionError("no circle of %d nodes at k = %d" % (nodes, k))


# a path of p rows takes ceil(log2(p - 1)) doubling rounds that move: 17, 129, 513, 2049 and 4097 add the round
# counts 4, 7, 9, 11 and 12, so that every count from 0 to 13 occurs
PATH_NODES = (1, 2, 3, 4, 5, 8, 9, 17, 32, 33, 63, 64, 65, 129, 255, 256, 257, 513, 1024, 1025, 2049, 4097, 5000)


def all_kmers(k: int):
    out = [""]
    for _ in range(k):
        out = [w + b for w in out for b in "ACGT"]
    return out


def cases() -> dict:
    """name -> (records, k, min_count): the named shapes; `both_strands`
    doubles each of them."""
    c = {}
    c["empty"] = ([("e", "ACGTNNACNNGT")], 21, 1)
    c["one_kmer"] = ([("o", path_seq(1, 21, 1))], 21, 1)
    for n in PATH_NODES:
        c["path_%d" % n] = ([("p", path_seq(n, 21, 100 + n))], 21, 1)
    c["all_3mers"] = ([("a%d" % i, w) for i, w in enumerate(all_kmers(3))], 3, 1)
    c["all_5mers"] = ([("a%d" % i, w) for i, w in enumerate(all_kmers(5))], 5, 1)
    c["acgt_k3"] = ([("h", "ACGT")], 3, 1)  # the hairpin: ACG and CGT are one row
    c["poly_a_alone"] = ([("a", "A" * 30)], 21, 1)
    c["poly_a_with_neighbours"] = ([("a", path_seq(40, 21, 7) + "A" * 30 + path_seq(40, 21, 8))], 21, 1)
    c["hairpin_k5"] = ([("h", "GGACGTCC"), ("i", "TTACGTAA")], 5, 1)
    stem, a, b = path_seq(60, 21, 11), path_seq(50, 21, 12), path_seq(70, 21, 13)
    c["y_fork"] = ([("s_a", stem + a), ("s_b", stem + b)], 21, 1)
    c["merge"] = ([("a_s", a + stem), ("b_s", b + stem)], 21, 1)
    c["fork_and_merge"] = ([("x", a + stem + b), ("y", path_seq(20, 21, 14) + stem + path_seq(20, 21, 15))], 21, 1)
    trunk = path_seq(120, 21, 21)
    tip = trunk[:60] + ("A" if trunk[60] != "A" else "C") + path_seq(1, 21, 22)[:8]
    c["tip_removed_by_L2"] = ([("t1", trunk), ("t2", trunk), ("tip", tip)], 21, 2)
    c["tip_kept"] = ([("t1", trunk), ("t2", trunk), ("tip", tip)], 21, 1)
    for n in (2, 3, 500):
        c["cycle_%d" % n] = ([("c", cycle_seq(n, 21 if n > 3 else 5, 30 + n))], 21 if n > 3 else 5, 1)
    cyc = cycle_seq(64, 21, 41)
    c["cycle_with_tail"] = ([("c", cyc), ("t", path_seq(30, 21, 42) + cyc[10:31])], 21, 1)
    c["two_cycles_and_paths"] = ([("c1", cycle_seq(256, 21, 51)), ("p1", path_seq(300, 21, 52)),
                                  ("c2", cycle_seq(37, 21, 53)), ("p2", path_seq(65, 21, 54)),
                                  ("p3", path_seq(1, 21, 55))], 21, 1)
    return c


def both_strands(records):
    """The records and their reverse complements: the same canonical table
    with every count doubled."""
    return list(records) + [(n + "_rc", sc.revcomp(s.upper())) for n, s in records]


def reverse_strand(records):
    """Every record reverse-complemented: the same canonical table."""
    return [(n, sc.revcomp(s.upper()) if "N" not in s.upper() else s) for n, s in records]
