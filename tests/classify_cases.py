"""`kmer classify` test helper (not a conftest): a plain-Python statement of
engine.color_table, kman_classify_records, kman_classify_pick,
engine.classify_assign, kman_format_classify and the command's --summary and
--reads-out-prefix files (include/kman.h), independent of the code under test.
It builds on tests/screen_cases.py (records, windows, keys) and, for the cut
files, on tests/reads_cases.py.

A reference is a list of ``(name, sequence)`` records; reference c is bit c of
a k-mer's mask.
"""

from __future__ import annotations

import os

import numpy as np

import reads_cases as rc
import screen_cases as sc

NONE = 0xFFFFFFFF
UNASSIGNED, AMBIGUOUS = -1, -2
M32 = (1 << 32) - 1


def color_table_of(refs, k: int, canonical: bool = False, min_count: int = 1, max_count=None) -> dict:
    """k-mer -> mask: bit c set when reference c holds the k-mer with a count
    (in that reference alone) within [min_count, max_count]."""
    t = {}
    for c, records in enumerate(refs):
        for w in sc.table_of(records, k, canonical, min_count, max_count):
            t[w] = t.get(w, 0) | (1 << c)
    return t


def table_rows(ctable: dict):
    """The coloured table as key-sorted rows: (u64 keys, u64 masks)."""
    rows = sorted((sc.key_of(w), m) for w, m in ctable.items())
    return (np.asarray([r[0] for r in rows], dtype=np.uint64), np.asarray([r[1] for r in rows], dtype=np.uint64))


def planes(records, k: int, ctable: dict, n_colors: int, canonical: bool = False, specific: bool = False):
    """kman_classify_records' planes, a (1 + n_colors, n_records) u32 array:
    row 0 the valid windows, row 1 + c the windows whose k-mer's mask, cut to
    its bits < n_colors, has bit c set (specific: is 1 << c exactly)."""
    cut = (1 << n_colors) - 1
    out = [[0] * len(records) for _ in range(1 + n_colors)]
    for r, (_, seq) in enumerate(records):
        ws = sc.windows(seq, k, canonical)
        out[0][r] = len(ws)
        for w in ws:
            m = ctable.get(w, 0) & cut
            if specific and m & (m - 1):
                continue
            c = 0
            while m:
                if m & 1:
                    out[1 + c][r] += 1
                m >>= 1
                c += 1
    return np.asarray([[v & M32 for v in row] for row in out], dtype=np.uint32).reshape(1 + n_colors, len(records))


def pick(hit_planes):
    """kman_classify_pick of (n_colors, n_records) hits, a (3, n_records) u32
    array: the lowest-indexed colour with the largest count (NONE when that is
    0), that count, and the largest count among the other colours."""
    hp = np.asarray(hit_planes, dtype=np.uint32)
    nc, R = hp.shape
    out = np.zeros((3, R), dtype=np.uint32)
    for r in range(R):
        col = [int(x) for x in hp[:, r]]
        best = max(col)
        c = col.index(best)
        others = col[:c] + col[c + 1:]
        out[:, r] = (c if best else NONE, best, max(others) if others else 0)
    return out


def assign(windows, best, hits, second, min_hits: int = 1, min_frac: float = 0.0, min_margin: int = 1) -> list:
    """-1 when hits < max(min_hits, 1) or hits < min_frac * windows, else -2
    when hits - second < min_margin, else best."""
    res = []
    for w, b, h, s in zip(*(np.asarray(a).tolist() for a in (windows, best, hits, second))):
        if h < max(min_hits, 1) or float(h) < min_frac * float(w):
            res.append(UNASSIGNED)
        elif h - s < min_margin:
            res.append(AMBIGUOUS)
        else:
            res.append(int(b))
    return res


def label_of(path: str) -> str:
    """The file's basename minus a trailing .gz and then one extension."""
    name = os.path.basename(path)
    if name.endswith(".gz"):
        name = name[:-3]
    return os.path.splitext(name)[0]


def lines(records, labels, windows, assigned, hits, second, hit_planes=None, kept=None) -> bytes:
    """NAME, K-MERS, LABEL, HITS, SECOND and, with hit_planes ((n_colors,
    n_records)), one column per reference."""
    out = []
    for r, (name, _) in enumerate(records):
        if kept is not None and not kept[r]:
            continue
        a = int(assigned[r])
        lab = labels[a] if a >= 0 else ("?" if a == AMBIGUOUS else "-")
        cols = [name, str(int(windows[r])), lab, str(int(hits[r])), str(int(second[r]))]
        if hit_planes is not None:
            cols += [str(int(x)) for x in np.asarray(hit_planes)[:, r]]
        out.append("\t".join(cols) + "\n")
    return "".join(out).encode()


def summary(labels, table_kmers, assigned) -> bytes:
    a = [int(x) for x in assigned]
    out = ["%s\t%d\t%d\n" % (lab, n, a.count(c)) for c, (lab, n) in enumerate(zip(labels, table_kmers))]
    out += ["?\t0\t%d\n" % a.count(AMBIGUOUS), "-\t0\t%d\n" % a.count(UNASSIGNED)]
    return "".join(out).encode()


def cut_files(text: bytes, offsets, labels, assigned, prefix: str, ext: str) -> dict:
    """path -> bytes of every --reads-out-prefix file: the records of `text`
    (offsets: reads_cases.fasta_offsets / fastq_offsets) by assignment."""
    a = [int(x) for x in assigned]
    files = {"%s.%s.%s" % (prefix, lab, ext): rc.cut_whole(text, offsets, [x == c for x in a])
             for c, lab in enumerate(labels)}
    files["%s.ambiguous.%s" % (prefix, ext)] = rc.cut_whole(text, offsets, [x == AMBIGUOUS for x in a])
    files["%s.unassigned.%s" % (prefix, ext)] = rc.cut_whole(text, offsets, [x == UNASSIGNED for x in a])
    return files


def classify(records, labels, refs, k, canonical=False, specific=False, min_count=1, max_count=None, min_hits=1,
             min_frac=0.0, min_margin=1):
    """The whole command on records: (planes, pick, assigned, table_kmers)."""
    ct = color_table_of(refs, k, canonical, min_count, max_count)
    pl = planes(records, k, ct, len(refs), canonical, specific)
    pk = pick(pl[1:])
    a = assign(pl[0], pk[0], pk[1], pk[2], min_hits, min_frac, min_margin)
    kmers = [len(sc.table_of(r, k, canonical, min_count, max_count)) for r in refs]
    return pl, pk, a, kmers


# ------------------------------------------------------------------ builders


def substring_refs(records, n_refs: int, seed: int = 1, pieces: int = 3, length: int = 90):
    """n_refs references, each a few random substrings of the reads'
    sequences; the substrings of different references overlap, so k-mers are
    held by several."""
    rng = np.random.default_rng(seed)
    seqs = [s for _, s in records if len(s) >= 8]
    refs = []
    for c in range(n_refs):
        recs = []
        for j in range(pieces):
            s = seqs[int(rng.integers(0, len(seqs)))]
            n = min(len(s), length)
            a = int(rng.integers(0, len(s) - n + 1))
            recs.append(("ref%d_%d" % (c, j), s[a:a + n]))
        refs.append(recs)
    return refs
