"""k > 32 test helper (not a conftest): a plain-Python statement, over byte
strings and Python ints, of what the word-key entry points compute
(include/kman.h: kman_extract_wide / kman_extract_words, kman_rle_wide /
kman_rle_words, kman_format_*_wide / *_words and their *_dev twins),
independent of the code under test, and the inputs that put events and
chosen keys at the kernels' tile edges.

  parse        FASTA text -> [(name, cleaned sequence)]  (parsers.py:86-128,
               batcher.py:551)
  windows      the stream of (k-mer bytes, pos) of kman_extract_*: valid
               windows in stream order, pos = (global base << 1) | strand
               (seq.py:285-328; strand 1 = the reverse complement, 274-282)
  to_words /   a k-mer as W = ceil(k / 32) ints, MSB-first, word 0 the first
  from_words   k - 32 (W - 1) bases
  rle          count: (key, group size); uniq: groups of one with their value
               (join.py:95-130, 244-285)
  count_text   "%s\\t%d\\n"                      (join.py:283-284)
  uniq_text    ">name:start-end:strand\\nSEQ\\n", start = the window's offset
               in its record, end = start + k    (seq.py:103-104, 489-495)
"""

from __future__ import annotations

import bisect
import random
import re

_WS = b" \t\n\x0b\x0c\r\x1c\x1d\x1e\x1f"  # what str.rstrip() strips, over ASCII
_COMP = bytes.maketrans(b"ACGT", b"TGCA")
_DIGIT = bytes.maketrans(b"ACGT", b"0123")
_BASES = b"ACGT"

TILE = 2048  # window starts per tile of both extraction kernels (ET * WEI, XT * XE)
PER_THREAD = 8
RLE_WIDE_TILE, RLE_WIDE_PER = 4096, 16  # rows per tile / thread of kman_rle_wide
RLE_WORDS_TILE, RLE_WORDS_PER = 2048, 8  # and of kman_rle_words
ONES = (1 << 64) - 1


def revcomp(w: bytes) -> bytes:
    return w.translate(_COMP)[::-1]


def nwords(k: int) -> int:
    return (k + 31) // 32


# ------------------------------------------------------------------- parsing
def parse(text: bytes):
    """[(name, cleaned sequence)]: universal newlines; a line starting with
    '>' opens a record (title = the rest, right-stripped; name = the title up
    to its first space); other lines of a record are right-stripped and
    joined, then blanks and CRs inside them dropped; lines before the first
    record are ignored."""
    recs = []
    for line in re.split(rb"\r\n|\r|\n", text):
        if line[:1] == b">":
            title = line[1:].decode("utf-8", "surrogateescape").rstrip()
            recs.append([title.split(" ")[0].encode("utf-8", "surrogateescape"), []])
        elif recs:
            recs[-1][1].append(line.rstrip(_WS))
    if not recs:
        raise AssertionError("premature end of file or empty file")
    return [(n, b"".join(s).replace(b" ", b"").replace(b"\r", b"")) for n, s in recs]


def rec_starts(records):
    """Global base index of every record's first base."""
    out, at = [], 0
    for _, s in records:
        out.append(at)
        at += len(s)
    return out


def fasta(records, width: int = 61) -> bytes:
    """FASTA text of [(name, sequence)], sequence lines of `width`."""
    parts = []
    for name, s in records:
        parts.append(b">" + name + b"\n")
        parts.extend(s[i:i + width] + b"\n" for i in range(0, len(s), width))
    return b"".join(parts)


# ---------------------------------------------------------------- extraction
def valid_starts(records, k: int):
    """(global base index, upper-case window) of every valid window: k
    characters of ACGT inside one record."""
    out, base = [], 0
    for _, s in records:
        u = s.upper()
        bad = -1  # the last index <= i + k - 1 that is not ACGT
        nxt = 0
        for i in range(len(u) - k + 1):
            while nxt < i + k:
                if u[nxt] not in _BASES:
                    bad = nxt
                nxt += 1
            if bad < i:
                out.append((base + i, u[i:i + k]))
        base += len(s)
    return out


def windows(records, k: int, rc: bool = False, canonical: bool = False):
    """[(k-mer, pos)] in stream order.  canonical wins over rc."""
    out = []
    for g, w in valid_starts(records, k):
        if canonical:
            out.append((min(w, revcomp(w)), g << 1))
        else:
            out.append((w, g << 1))
            if rc:
                out.append((revcomp(w), (g << 1) | 1))
    return out


def to_words(kmer: bytes):
    k = len(kmer)
    h = k - 32 * (nwords(k) - 1)
    cuts = [0, h] + list(range(h + 32, k + 1, 32))
    return tuple(int(kmer[a:b].translate(_DIGIT), 4) for a, b in zip(cuts, cuts[1:]))


def from_words(words, k: int) -> bytes:
    W = nwords(k)
    assert len(words) == W
    h = k - 32 * (W - 1)
    out = bytearray()
    for j, w in enumerate(words):
        n = h if j == 0 else 32
        assert 0 <= w < 1 << (2 * n)
        out += bytes(_BASES[(w >> (2 * (n - 1 - t))) & 3] for t in range(n))
    return bytes(out)


# ---------------------------------------------------------------- run-length
def rle(rows, vals, mode: str):
    """rows: sorted keys (anything comparable with ==: bytes or word tuples).
    count -> ([key], [group size]); uniq -> ([key], [value]) of groups of one.
    Groups are runs of equal neighbours."""
    keys, out = [], []
    i, n = 0, len(rows)
    while i < n:
        j = i + 1
        while j < n and rows[j] == rows[i]:
            j += 1
        if mode == "count":
            keys.append(rows[i])
            out.append(j - i)
        elif j - i == 1:
            keys.append(rows[i])
            out.append(vals[i])
        i = j
    return keys, out


# ------------------------------------------------------------------- writers
def count_text(rows, counts, k: int) -> bytes:
    assert all(len(r) == k for r in rows)
    return b"".join(b"%s\t%d\n" % (r, c) for r, c in zip(rows, counts))


def uniq_text(rows, pos, k: int, names, rec_seq) -> bytes:
    """rec_seq: ascending first-base indices; the record of base g is the last
    one whose first base is <= g."""
    out = []
    for r, p in zip(rows, pos):
        assert len(r) == k
        g = p >> 1
        rec = bisect.bisect_right(rec_seq, g) - 1
        st = g - rec_seq[rec]
        out.append(b">%s:%d-%d:%s\n%s\n" % (names[rec], st, st + k, b"-" if p & 1 else b"+", r))
    return b"".join(out)


def restate(text: bytes, k: int, mode: str, rc: bool = False, canonical: bool = False) -> bytes:
    """`kmer count` / `kmer uniq` output of a FASTA text."""
    recs = parse(text)
    ws = sorted(windows(recs, k, rc, canonical), key=lambda x: x[0])  # (stable: ties keep stream order)
    keys, vals = rle([w for w, _ in ws], [p for _, p in ws], mode)
    if mode == "count":
        return count_text(keys, vals, k)
    return uniq_text(keys, vals, k, [n for n, _ in recs], rec_starts(recs))


# ------------------------------------------------------------ input builders
def clean(n: int, seed) -> bytes:
    rng = random.Random("clean/%s" % (seed,))
    return bytes(rng.choices(_BASES, k=n))


SEQ_LEN3 = 3 * TILE + 5  # the clean 3-tile record


def lengths(k: int):
    return [k - 1, k, k + 1, TILE - 1, TILE, TILE + 1, TILE + k - 1, TILE + k, SEQ_LEN3]


def event_offsets(k: int):
    return [T + d for T in (TILE, 2 * TILE) for d in (-k, -k + 1, -8, -1, 0, 1, 7, 8, k - 1)]


def with_n(at: int, seed=0):
    """One clean 3-tile record with an N at base index `at`."""
    s = bytearray(clean(SEQ_LEN3, seed))
    s[at] = ord("N")
    return [(b"n%d" % at, bytes(s))]


def with_start(at: int, seed=0):
    """The same bases cut in two records: the second starts at base `at`."""
    s = clean(SEQ_LEN3, seed)
    return [(b"a", s[:at]), (b"b%d" % at, s[at:])]


def two_events(k: int, between: int, at: int = TILE - 40, second_is_start: bool = False, seed=0):
    """An N at `at`, then `between` clean bases, then a second event (an N, or
    a record start): between = k - 1 leaves no window between them, k one."""
    s = bytearray(clean(SEQ_LEN3, seed))
    s[at] = ord("N")
    e = at + 1 + between
    if second_is_start:
        return [(b"a", bytes(s[:e])), (b"b", bytes(s[e:]))]
    s[e] = ord("N")
    return [(b"t", bytes(s))]


def palindrome(k: int, seed=0) -> bytes:
    """A reverse-complement palindrome (even k)."""
    assert k % 2 == 0
    h = clean(k // 2, "pal%d/%s" % (k, seed))
    return h + revcomp(h)


def hi_tie(k: int, forward_wins: bool, seed=0) -> bytes:
    """A window (33 <= k < 64) whose first k - 32 bases equal the reverse
    complement of its last k - 32, so the first word of the window and of its
    reverse complement are equal and the 32-base word decides."""
    assert 33 <= k < 64
    m = k - 32
    a = clean(m, "tie%d/%s" % (k, seed))
    for t in range(1000):
        mid = clean(k - 2 * m, "mid%d/%s/%d" % (k, seed, t))
        if mid != revcomp(mid) and (mid < revcomp(mid)) == forward_wins:
            return a + mid + revcomp(a)
    raise AssertionError("no middle found")


def embed(window: bytes, at: int, seed=0):
    """One clean 3-tile record with `window` at base index `at`."""
    s = bytearray(clean(SEQ_LEN3, seed))
    s[at:at + len(window)] = window
    assert len(s) == SEQ_LEN3
    return [(b"e%d" % at, bytes(s))]


# ---------------------------------------------------- run-length row layouts
def _heads_to_sizes(head):
    sizes = []
    for h in head:
        if h or not sizes:
            sizes.append(1)
        else:
            sizes[-1] += 1
    return sizes


def rle_layouts(n: int, tile: int, per: int):
    """{name: group sizes summing to n}: the layouts that put group ends at
    the edges of a kernel's tiles (`tile` rows) and of a thread's `per` rows."""
    out = {}
    if n == 0:
        return {"empty": []}
    out["distinct"] = [1] * n
    out["equal"] = [n]
    base = [i % 3 == 0 for i in range(n)]
    # a group of exactly 2 straddling each tile boundary
    head = list(base)
    for b in range(tile, n, tile):
        head[b - 1], head[b] = True, False
        if b + 1 < n:
            head[b + 1] = True
    out["straddle2"] = _heads_to_sizes(head)
    # one group over two whole tiles plus one row on each side (clipped to n)
    if n > tile:
        a, e = tile - 1, min(n, 3 * tile + 1)
        out["long"] = [1] * a + [e - a] + [1] * (n - e)
    # singletons at the first and last row of a tile and of a thread's rows
    head = list(base)
    marks = set()
    for t in range(0, n, tile):
        marks.update((t, t + tile - 1, t + 5 * per, t + 6 * per - 1))
    for i in sorted(marks):
        if i < n:
            head[i] = True
            if i + 1 < n:
                head[i + 1] = True
    out["singles"] = _heads_to_sizes(head)
    # a group that ends at row n - 1
    if n >= 3:
        out["tail"] = [1] * (n - 3) + [3]
    for s in out.values():
        assert sum(s) == n and all(x > 0 for x in s)
    return out


_C = 0x0123456789ABCDEF


def _mixw(g: int, q: int) -> int:
    x = (g * 0x9E3779B97F4A7C15 + q * 0xD1B54A32D192ED03 + 1) & ONES
    x ^= x >> 29
    return (x * 0xBF58476D1CE4E5B9) & ONES


def rle_rows(sizes, W: int, vary="all", ones=""):
    """Rows (W-word tuples) of the groups: group g's key differs from its
    neighbours' in word `vary` only (an int), or in every word ("all"); keys
    ascend with g where `vary` is an int.  ones: "first" / "last" / "both"
    gives those groups (they must be groups of one) the key with every word
    ~0."""
    rows = []
    G = len(sizes)
    for g, m in enumerate(sizes):
        if vary == "all":
            key = tuple(_mixw(g, q) >> 1 for q in range(W))  # (bit 63 clear: never the all-ones key)
        else:
            key = tuple(g + 1 if q == vary else _C for q in range(W))
        if (g == 0 and ones in ("first", "both")) or (g == G - 1 and ones in ("last", "both")):
            assert m == 1
            key = (ONES,) * W
        rows.extend([key] * m)
    return rows
