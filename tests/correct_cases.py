"""`kmer screen --correct` test helper (not a conftest): a plain-Python
statement of kman_correct_sites, kman_apply_fixes and
kman_format_screen_correct (include/kman.h), independent of the code under
test, built on screen_cases, median_cases.window_words, solid_cases and
reads_cases.

The rule, for record r with bases [s, e) and the words wc of
kman_window_counts on these codes, this table, k, flags and threshold C:
window start b is weak when wc[b] != NONE and wc[b] < C, solid when wc[b] !=
NONE and wc[b] >= C.  A weak run [a, b) is a maximal interval of weak window
starts inside the record.  L = a > s and a - 1 solid; R = b <= e - k and b
solid; openL = a == s; openR = b == e - k + 1.  The run names the site
    L and R,     b - a == k   p = b - 1
    L and openR, b - a <= k   p = a + k - 1
    openL and R, b - a <= k   p = b - 1
and nothing else does.  With o the base at p, ok(x) for x != o: every window
of the run, with x at p, has a count >= C in the table (the canonical k-mer
under `canonical`).  The site is corrected to x when exactly one x is ok.
"""

from __future__ import annotations

import re

import median_cases as mc
import reads_cases as rc
import screen_cases as sc
import solid_cases as so

NONE = mc.NONE
NOFIX = 0xFF  # KMAN_FIX_NONE
_TERM = re.compile(rb"\r\n|\n|\r")


def weak(word: int, C: int) -> bool:
    return int(word) != NONE and int(word) < C


def solid(word: int, C: int) -> bool:
    return int(word) != NONE and int(word) >= C


def weak_runs(words, s: int, e: int, C: int) -> list:
    """The maximal intervals [a, b) of weak words inside [s, e)."""
    out, b = [], s
    while b < e:
        if not weak(words[b], C):
            b += 1
            continue
        a = b
        while b < e and weak(words[b], C):
            b += 1
        out.append((a, b))
    return out


def site_of(words, a: int, b: int, s: int, e: int, k: int, C: int):
    """The base that the weak run [a, b) of the record [s, e) names, or None."""
    L = a > s and solid(words[a - 1], C)
    R = b <= e - k and solid(words[b], C)
    open_l, open_r = a == s, b == e - k + 1
    if L and R:
        return b - 1 if b - a == k else None
    if L and open_r:
        return a + k - 1 if b - a <= k else None
    if open_l and R:
        return b - 1 if b - a <= k else None
    return None


def count_of(kmer: str, table: dict, canonical: bool) -> int:
    return table.get(min(kmer, sc.revcomp(kmer)) if canonical else kmer, 0)


def fix_plane(codes, words, rec_seq, n_bases: int, k: int, table: dict, C: int, canonical: bool = False) -> list:
    """kman_correct_sites' d_fix: one value per base, NOFIX or the new base.
    codes: the parsers' codes (bits 0-1 the base); table: k-mer -> count."""
    fix = [NOFIX] * n_bases
    rs = [min(int(x), n_bases) for x in rec_seq] + [n_bases]
    for r in range(len(rs) - 1):
        s, e = rs[r], rs[r + 1]
        for a, b in weak_runs(words, s, e, C):
            p = site_of(words, a, b, s, e, k, C)
            if p is None:
                continue
            o = int(codes[p]) & 3
            good = []
            for x in range(4):
                if x == o:
                    continue
                seq = ["ACGT"[int(c) & 3] for c in codes[a:b + k - 1]]
                seq[p - a] = "ACGT"[x]
                if all(count_of("".join(seq[w - a:w - a + k]), table, canonical) >= C for w in range(a, b)):
                    good.append(x)
            if len(good) == 1:
                fix[p] = good[0]
    return fix


def named_sites(words, rec_seq, n_bases: int, k: int, C: int) -> list:
    """The bases that the weak runs name, corrected or not, ascending."""
    rs = [min(int(x), n_bases) for x in rec_seq] + [n_bases]
    out = []
    for r in range(len(rs) - 1):
        for a, b in weak_runs(words, rs[r], rs[r + 1], C):
            p = site_of(words, a, b, rs[r], rs[r + 1], k, C)
            if p is not None:
                out.append(p)
    return out


def fix_plane_of(records, k: int, table: dict, C: int, canonical: bool = False) -> list:
    """fix_plane over the records' own codes and window words."""
    codes, rec_seq, n = sc.codes_of(records)
    return fix_plane(codes[:n].tolist(), mc.window_words(records, k, table, canonical), rec_seq, n, k, table, C,
                     canonical)


def apply_codes(codes, fix) -> list:
    """codes[b] = fix[b] | (codes[b] & 8) where fix[b] != NOFIX."""
    return [int(c) if f == NOFIX else (int(f) | (int(c) & 8)) for c, f in zip(codes, fix)]


def nfix(fix, rec_seq, n_bases: int) -> list:
    rs = [min(int(x), n_bases) for x in rec_seq] + [n_bases]
    return [sum(1 for f in fix[rs[r]:max(rs[r], rs[r + 1])] if f != NOFIX) for r in range(len(rs) - 1)]


def corrected(records, fix) -> list:
    """The records with their fixed bases replaced (upper case: what the codes hold)."""
    out, at = [], 0
    for name, seq in records:
        s = list(seq)
        for i in range(len(s)):
            if fix[at + i] != NOFIX:
                s[i] = "ACGT"[fix[at + i]]
        out.append((name, "".join(s)))
        at += len(seq)
    return out


def apply_text(text: bytes, off, rec_seq, fix, n_bases: int) -> bytes:
    """The four-line FASTQ text with the fixed bases replaced: in record r
    (bytes [off[r], off[r + 1])) the i-th kept character of the second line
    (reads_cases.cols_of) is base rec_seq[r] + i; a fixed one becomes
    "ACGT"[x], lower case when the byte it replaces is a lower-case letter."""
    out = bytearray(text)
    o = rc.clamp_offsets(off, len(text))
    rs = [min(int(x), n_bases) for x in rec_seq] + [n_bases]
    for r in range(len(o) - 1):
        rec = text[o[r]:max(o[r], o[r + 1])]
        m = _TERM.search(rec)
        if m is None:
            continue
        l2 = _TERM.split(rec[m.end():])[0]
        for i, c in enumerate(rc.cols_of(l2)):
            b = rs[r] + i
            if b < rs[r + 1] and fix[b] != NOFIX:
                at = o[r] + m.end() + c
                old = text[at:at + 1]
                new = b"ACGT"[fix[b]:fix[b] + 1]
                out[at:at + 1] = new.lower() if old.islower() else new
    return bytes(out)


def lines(records, st, span, fixes, med=None, kept=None) -> bytes:
    """kman_format_screen_correct: solid_cases.lines with FIXES as the last column."""
    out = []
    for r, (name, _) in enumerate(records):
        if kept is None or kept[r]:
            cols = [name] + [str(int(x)) for x in st[r]]
            if med is not None:
                cols.append(str(int(med[r])))
            cols += [str(int(span[r][0])), str(int(span[r][1])), str(int(fixes[r]))]
            out.append(("\t".join(cols) + "\n").encode())
    return b"".join(out)


def screen_of(records, k: int, table: dict, C: int, canonical: bool = False):
    """What `kmer screen --solid C --correct` reports: (the corrected records,
    stats, span, fixes per record), every column from the corrected records."""
    fix = fix_plane_of(records, k, table, C, canonical)
    _, rec_seq, n = sc.codes_of(records)
    fixed = corrected(records, fix)
    span = so.spans(so.runs_of(fixed, k, table, C, canonical), k)
    return fixed, sc.stats(fixed, k, table, canonical), span, nfix(fix, rec_seq, n)


# ------------------------------------------------------------------ builders


def sub(seq: str, at: int, step: int = 1) -> str:
    """seq with the base at `at` replaced by the one `step` further in ACGT."""
    return seq[:at] + "ACGT"[("ACGT".index(seq[at]) + step) % 4] + seq[at + 1:]


def kmer_table(seqs, k: int, canonical: bool = False, count: int = 5) -> dict:
    """The k-mers of the sequences, every one with the same count."""
    return {w: count for w in sc.table_of([("", s) for s in seqs], k, canonical)}


# Genomes of 4 k + 4 bases for the hand cases.  k = 3 and 4: chosen so that no
# k-mer that a substitution of the cases below creates is a k-mer of the
# genome (test_correct_cpu checks every expectation and every designed weak
# run against the statement); k = 4 on both strands, k = 3 on the forward
# strand alone (16 bases hold 14 of the 32 canonical 3-mers: no genome keeps
# them apart).  Larger k: random, where such a coincidence has no chance.
HAND_GENOMES = {3: "AGTCTTACAGTCGATG", 4: "CCATCTTTCACTTGCGGCTC"}


def hand_genome(k: int) -> str:
    import numpy as np

    return HAND_GENOMES.get(k) or sc.rand_seq(np.random.default_rng(100 + k), 4 * k + 4)


def hand_cases(k: int, canonical: bool = False, C: int = 3, genome=None) -> list:
    """(name, records, table, C, expected) with expected = {global base index:
    new base}: what the rule gives by construction, worked out by hand from
    where the errors were put, not by running the statement."""
    g = genome or hand_genome(k)
    e = len(g)
    assert e == 4 * k + 4
    full = kmer_table([g], k, canonical)
    code = {c: i for i, c in enumerate("ACGT")}
    cases = []

    def one(name, read, expected, table=full, c=C):
        cases.append((name, [("r", read)], table, c, expected))

    m = 2 * k
    one("clean", g, {})
    one("interior", sub(g, m), {m: code[g[m]]})
    one("first_base", sub(g, 0), {0: code[g[0]]})
    one("last_base", sub(g, e - 1), {e - 1: code[g[e - 1]]})
    one("column_k_minus_1", sub(g, k - 1, 2), {k - 1: code[g[k - 1]]})
    one("column_e_minus_k", sub(g, e - k, 3), {e - k: code[g[e - k]]})
    one("two_more_than_k_apart", sub(sub(g, k), 2 * k + 1, 2), {k: code[g[k]], 2 * k + 1: code[g[2 * k + 1]]})
    one("two_exactly_k_apart", sub(sub(g, k + 1), 2 * k + 1), {})   # one weak run of 2 k
    one("two_closer_than_k", sub(sub(g, k + 1), k + 3), {})          # one weak run of k + 2
    one("two_alternatives_ok", sub(g, m, 2), {}, kmer_table([g, sub(g, m, 1)], k, canonical))
    # the table lacks every window over m: nothing fits there, the read's own base included
    no_alt = kmer_table([g[:m], g[m + 1:]], k, canonical)
    one("no_alternative_ok", g, {}, no_alt)
    one("run_touching_an_N", sub(g, m)[:m + k] + "N" + g[m + k + 1:], {})
    one("record_of_k_bases", sub(g[:k], 1), {})
    # records shorter than k and empty ones between two reads with an error each
    recs = [("a", sub(g, m)), ("b", g[:k - 1]), ("c", ""), ("d", "A"), ("e", ""), ("f", sub(g, 0, 2)), ("g", "")]
    cases.append(("short_and_empty_records", recs, full, C, {m: code[g[m]], e + k: code[g[0]]}))
    # the threshold: a count of exactly C is solid and ok, C - 1 is neither
    one("count_C", sub(g, m), {m: code[g[m]]}, kmer_table([g], k, canonical, C))
    one("count_C_minus_1", sub(g, m), {}, kmer_table([g], k, canonical, C - 1))
    low = dict(full)
    w = g[m:m + k]
    low[min(w, sc.revcomp(w)) if canonical else w] = C - 1
    one("candidate_window_at_C_minus_1", sub(g, m), {}, low)
    return cases


def hand_runs(k: int) -> dict:
    """The weak runs that some of the hand cases are built to have."""
    e = 4 * k + 4
    return {"clean": [], "interior": [(k + 1, 2 * k + 1)], "first_base": [(0, 1)], "last_base": [(e - k, e - k + 1)],
            "column_k_minus_1": [(0, k)], "column_e_minus_k": [(e - 2 * k + 1, e - k + 1)],
            "two_more_than_k_apart": [(1, k + 1), (k + 2, 2 * k + 2)], "two_exactly_k_apart": [(2, 2 * k + 2)],
            "two_closer_than_k": [(2, k + 4)], "two_alternatives_ok": [(k + 1, 2 * k + 1)],
            "no_alternative_ok": [(k + 1, 2 * k + 1)], "run_touching_an_N": [(k + 1, 2 * k + 1)],
            "record_of_k_bases": [(0, 1)], "count_C": [(k + 1, 2 * k + 1)], "count_C_minus_1": [(0, e - k + 1)],
            "candidate_window_at_C_minus_1": [(k + 1, 2 * k + 1)]}


def expected_plane(n_bases: int, expected: dict) -> list:
    fix = [NOFIX] * n_bases
    for b, x in expected.items():
        fix[b] = x
    return fix


def random_case(seed: int = 7, genome_len: int = 2000, n_reads: int = 200, read_len: int = 100, rate: float = 0.015):
    """(genome, reads, the error-free reads): reads of one random genome, every
    base substituted with probability `rate`."""
    import numpy as np

    rng = np.random.default_rng(seed)
    genome = sc.rand_seq(rng, genome_len)
    reads, clean = [], []
    for i in range(n_reads):
        at = int(rng.integers(0, genome_len - read_len + 1))
        s = genome[at:at + read_len]
        clean.append(("read%d" % i, s))
        hit = rng.random(read_len) < rate
        step = rng.integers(1, 4, read_len)
        s = "".join("ACGT"[("ACGT".index(c) + int(step[j])) % 4] if hit[j] else c for j, c in enumerate(s))
        reads.append(("read%d" % i, s))
    return genome, reads, clean
