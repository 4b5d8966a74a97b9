"""`kmer screen --median` test helper (not a conftest): a plain-Python
statement of kman_window_counts / kman_record_quantile /
kman_format_screen_median and of engine.screen_keep's median bounds
(include/kman.h), independent of the code under test, built on
screen_cases.windows / table_of.
"""

from __future__ import annotations

import numpy as np

import screen_cases as sc

NONE = 0xFFFFFFFF  # KMAN_WC_NONE
SAT = 0xFFFFFFFE   # the largest count a word holds


def window_words(records, k: int, table: dict, canonical: bool = False) -> list:
    """One word per base of the concatenated records: NONE where no valid
    window starts, else the window's count in `table` (absent: 0), saturated."""
    out = []
    for _, seq in records:
        for i in range(len(seq)):
            w = sc.windows(seq[i:i + k], k, canonical) if i + k <= len(seq) else []
            out.append(min(table.get(w[0], 0), SAT) if w else NONE)
    return out


def quantile(vals, num: int = 1, den: int = 2) -> int:
    """sorted(non-NONE words)[(w - 1) * num // den]; 0 when there is none."""
    v = sorted(int(x) for x in vals if int(x) != NONE)
    return v[(len(v) - 1) * num // den] if v else 0


def record_quantiles(words, rec_seq, n_bases: int, num: int = 1, den: int = 2) -> list:
    """The quantile of every record: record r owns [rec_seq[r], rec_seq[r + 1]),
    the last one runs to n_bases; entries are clamped to n_bases."""
    rs = [min(int(x), n_bases) for x in rec_seq] + [n_bases]
    return [quantile(words[rs[r]:max(rs[r], rs[r + 1])], num, den) for r in range(len(rs) - 1)]


def medians(records, k: int, table: dict, canonical: bool = False, num: int = 1, den: int = 2) -> list:
    out = []
    for rec in records:
        out.append(quantile(window_words([rec], k, table, canonical), num, den))
    return out


def keep(st, med, min_hits: int = 0, min_frac: float = 0.0, invert: bool = False, min_median=None, max_median=None):
    res = []
    for (w, h, _), m in zip(np.asarray(st).tolist(), med):
        ok = float(h) >= min_hits and float(h) >= min_frac * float(w)
        ok = ok and (min_median is None or int(m) >= min_median) and (max_median is None or int(m) <= max_median)
        res.append(bool(ok) != bool(invert))
    return res


def lines(records, st, med, kept=None) -> bytes:
    out = []
    for r, (name, _) in enumerate(records):
        if kept is None or kept[r]:
            w, h, s = (int(x) for x in st[r])
            out.append(("%s\t%d\t%d\t%d\t%d\n" % (name, w, h, s, int(med[r]))).encode())
    return b"".join(out)


def property_holds(st, med) -> bool:
    """median > 0 exactly when the record has windows and fewer than half of
    them (the lower median's side) are absent from the table (tables whose
    counts are all >= 1)."""
    for (w, h, _), m in zip(np.asarray(st).tolist(), med):
        if (int(m) > 0) != (w > 0 and w - h <= (w - 1) // 2):
            return False
    return True
