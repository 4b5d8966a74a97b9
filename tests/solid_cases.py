"""`kmer screen --solid` test helper (not a conftest): a plain-Python
statement of kman_record_runs, engine.solid_spans, engine.screen_keep's span
rule, kman_format_screen_solid and kman_format_bed (include/kman.h),
independent of the code under test, built on screen_cases and
median_cases.window_words.
"""

from __future__ import annotations

import numpy as np

import median_cases as mc
import screen_cases as sc

NONE = mc.NONE


def solid(word: int, min_count: int) -> bool:
    return int(word) != NONE and int(word) >= min_count


def longest_run(words, min_count: int):
    """(start, len) of the leftmost longest run of solid words; (0, 0) without one."""
    best_s = best_l = 0
    i, n = 0, len(words)
    while i < n:
        if not solid(words[i], min_count):
            i += 1
            continue
        j = i
        while j < n and solid(words[j], min_count):
            j += 1
        if j - i > best_l:  # (strictly longer: of equal runs the leftmost stays)
            best_s, best_l = i, j - i
        i = j
    return best_s, best_l


def record_runs(words, rec_seq, n_bases: int, min_count: int) -> list:
    """(start, len) per record: record r owns [rec_seq[r], rec_seq[r + 1]), the
    last one runs to n_bases; entries are clamped to n_bases; a run never
    leaves its record."""
    rs = [min(int(x), n_bases) for x in rec_seq] + [n_bases]
    return [longest_run(list(words[rs[r]:max(rs[r], rs[r + 1])]), min_count) for r in range(len(rs) - 1)]


def runs_of(records, k: int, table: dict, min_count: int, canonical: bool = False) -> list:
    """(start, len) per (name, sequence) record against a k-mer -> count table."""
    return [longest_run(mc.window_words([rec], k, table, canonical), min_count) for rec in records]


def spans(runs, k: int) -> list:
    """(START, END) in bases: a run of len windows covers len + k - 1 bases."""
    return [(int(s), int(s) + int(n) + k - 1) if int(n) > 0 else (0, 0) for s, n in runs]


def keep(st, span, min_hits: int = 0, min_frac: float = 0.0, invert: bool = False, min_solid_len=None, med=None,
         min_median=None, max_median=None):
    res = []
    for r, (w, h, _) in enumerate(np.asarray(st).tolist()):
        ok = float(h) >= min_hits and float(h) >= min_frac * float(w)
        if med is not None:
            ok = ok and (min_median is None or int(med[r]) >= min_median)
            ok = ok and (max_median is None or int(med[r]) <= max_median)
        ok = ok and (min_solid_len is None or span[r][1] - span[r][0] >= min_solid_len)
        res.append(bool(ok) != bool(invert))
    return res


def lines(records, st, span, med=None, kept=None) -> bytes:
    out = []
    for r, (name, _) in enumerate(records):
        if kept is None or kept[r]:
            cols = [name] + [str(int(x)) for x in st[r]]
            if med is not None:
                cols.append(str(int(med[r])))
            cols += [str(int(span[r][0])), str(int(span[r][1]))]
            out.append(("\t".join(cols) + "\n").encode())
    return b"".join(out)


def bed(records, span, kept=None) -> bytes:
    out = []
    for r, (name, _) in enumerate(records):
        if (kept is None or kept[r]) and span[r][1] > span[r][0]:
            out.append(("%s\t%d\t%d\n" % (name, span[r][0], span[r][1])).encode())
    return b"".join(out)


def cut(records, span) -> list:
    """The text a BED line selects: seq[START:END] of every record with a span."""
    return [seq[a:b] for (_, seq), (a, b) in zip(records, span) if b > a]
