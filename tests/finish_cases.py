"""Inputs for kman_finish (kman_amd/csrc/segsort.hip) at the edges of its
chunk geometry, in plain numpy.

layout() constructs a prefix-sorted key array from a list of segments, so
every position is known without running kman_sort_range.  plan() restates
what segfin_kernel decides for every chunk of such an array: the owned range,
the longest segment, the sort path, how the end of the last owned segment is
found, and which segments go through the big-segment fallback.  CASES names,
for every layout, the property it is there for; tests/test_finish_cases_cpu.py
holds plan() to those names, tests/test_gpu_finish_edges.py runs the table."""

from __future__ import annotations

import bisect
import functools
import zlib
from dataclasses import dataclass, field

import numpy as np

# segsort.hip: FC, FR, PI * FT, WI * 64
C, R, L, W = 5120, 6144, 5632, 768
FT = 512
U32_BITS = 22   # wave path: low bits <= 22 travel packed in 32 bits
WAVE_BITS = 51  # wave path: low bits <= 51 (13 position bits beside them)
DIGIT = 7

MASK64 = (1 << 64) - 1


@dataclass(frozen=True)
class Seg:
    """n keys of one prefix.  low: "distinct", "equal", ("pool", g) -- each
    key one of g values -- or ("groups", lengths): groups of those sizes, in
    ascending key order."""

    n: int
    low: object = "distinct"


def _distinct(cnt, bits, rng):
    """cnt distinct values of `bits` bits, ascending."""
    if cnt > (1 << bits):
        raise ValueError("%d distinct values do not fit %d bits" % (cnt, bits))
    if bits <= 16:
        return np.sort(rng.permutation(1 << bits)[:cnt].astype(np.uint64))
    got = np.zeros(0, np.uint64)
    while len(got) < cnt:
        d = rng.integers(0, 1 << min(bits, 63), size=2 * cnt + 8, dtype=np.uint64)
        if bits == 64:
            d = d * np.uint64(2) + rng.integers(0, 2, size=len(d)).astype(np.uint64)
        got = np.unique(np.concatenate([got, d]))
    return np.sort(got[rng.permutation(len(got))[:cnt]])


def _low(seg, bits, rng):
    kind = seg.low
    if kind == "distinct":
        v = _distinct(seg.n, bits, rng)
    elif kind == "equal":
        v = np.repeat(_distinct(1, bits, rng), seg.n)
    elif kind[0] == "pool":
        pool = _distinct(kind[1], bits, rng)
        v = pool[rng.integers(0, len(pool), size=seg.n)]
    elif kind[0] == "groups":
        lens = np.asarray(kind[1], dtype=np.int64)
        if lens.sum() != seg.n or (lens <= 0).any():
            raise ValueError("group lengths do not add up to the segment")
        v = np.repeat(_distinct(len(lens), bits, rng), lens)
    else:
        raise ValueError("unknown draw %r" % (kind,))
    return v[rng.permutation(seg.n)]


def layout(segments, lo_bit, key_bits, rng):
    """uint64 keys of key_bits bits: the segments in order, prefixes
    (key >> lo_bit) ascending over the whole prefix range, every segment's
    keys shuffled."""
    if not (1 <= key_bits <= 64 and 0 <= lo_bit <= key_bits):
        raise ValueError("bad key bits %d / low bit %d" % (key_bits, lo_bit))
    space = 1 << (key_bits - lo_bit)
    nseg = len(segments)
    if nseg == 0 or nseg > space:
        raise ValueError("%d segments need more than %d prefix bits" % (nseg, key_bits - lo_bit))
    parts = []
    for i, seg in enumerate(segments):
        if seg.n <= 0:
            raise ValueError("empty segment")
        pre = (i * space) // nseg  # strictly ascending: space >= nseg
        hi = np.uint64((pre << lo_bit) & MASK64) if lo_bit < 64 else np.uint64(0)
        parts.append(_low(seg, lo_bit, rng) | hi)
    return np.concatenate(parts)


def prefixes(keys, lo_bit):
    return np.zeros(len(keys), np.uint64) if lo_bit >= 64 else keys >> np.uint64(lo_bit)


# ---------------------------------------------------------------- the plan


@dataclass
class Chunk:
    tile: int
    cnt: int
    has_start: bool
    owned: int      # segments that start in the chunk
    first: int      # offset of the first start (None without one)
    lo: int
    hi: int
    nsegs: int      # segments of [lo, hi), presorted slices included
    maxlen: int     # longest of them (0 when nothing is sorted)
    path: str       # none | wave32 | wave64 | block | block0
    tail: str       # none | loaded | array_end | rounds | big
    lead_pre: bool
    trail_pre: bool


@dataclass
class Plan:
    chunks: list
    big: list       # (start, end) of the segments re-sorted through the fallback
    launches: int   # runs of segfin_kernel: 2 with a big segment


def _run(pre, start, n, lo_bit, ov):
    """One run of segfin_kernel over every chunk; ov = listed big segments."""
    starts_of = [s for s, _ in ov]
    chunks, found = [], []
    for tile in range((n + C - 1) // C):
        base = tile * C
        cnt = min(n - base, C)
        # the mask: starts among the keys loaded with the chunk
        st = np.flatnonzero(start[base:base + min(n - base, L)])
        own, beyond = st[st < cnt], st[st >= cnt]
        has_start = len(own) > 0
        first = int(own[0]) if has_start else None
        last = int(own[-1]) if has_start else None
        endp = int(beyond[0]) if len(beyond) else None
        lead_pre = last_pre = False
        if ov:
            if (first is None or first > 0) and base > 0:
                i = bisect.bisect_right(starts_of, base) - 1
                lead_pre = i >= 0 and ov[i][1] > base
            if has_start:
                i = bisect.bisect_right(starts_of, base + last) - 1
                last_pre = i >= 0 and ov[i][0] == base + last
        hi, trail_pre, tail = cnt, last_pre, "none"
        if has_start:
            if last_pre:
                tail = "big"
            elif base + cnt >= n:
                tail = "array_end"
            elif endp is not None:
                hi, tail = endp, "loaded"
            elif n - base <= L:
                hi, tail = n - base, "array_end"
            else:
                s_end = R + 1
                for r0 in range(L, R, FT):
                    for rel in range(r0, r0 + FT):
                        g = base + rel
                        if (g < n and pre[g] != pre[base + last]) or g == n:
                            s_end = min(s_end, rel)
                    if s_end < r0 + FT:
                        break
                if s_end > R:
                    found.append(base + last)  # (the first run: its range stops before the segment)
                    hi, tail = last, "big"
                else:
                    hi, tail = s_end, "rounds"
        lo = 0 if lead_pre else (first if has_start else cnt)
        if not has_start and not lead_pre:
            hi = lo
        m = hi - lo
        nsegs = maxlen = 0
        path = "none"
        if has_start and m > 1:
            inner = [int(x) for x in st if lo < x < hi]
            bounds = [lo] + inner + [hi]
            nsegs = len(bounds) - 1
            maxlen = max(b - a for a, b in zip(bounds, bounds[1:]))
            low_bits = min(lo_bit, 64)
            if maxlen <= W and low_bits <= WAVE_BITS:
                path = "wave32" if low_bits <= U32_BITS else "wave64"
            else:
                sbits = (nsegs - 1).bit_length()
                path = "block0" if sbits + low_bits == 0 else "block"
        chunks.append(Chunk(tile, cnt, has_start, len(own), first, lo, hi, nsegs, maxlen, path, tail, lead_pre,
                            trail_pre))
    return chunks, found


def plan(keys, lo_bit):
    keys = np.asarray(keys, dtype=np.uint64)
    n = len(keys)
    pre = prefixes(keys, lo_bit)
    start = np.ones(n, bool)
    start[1:] = pre[1:] != pre[:-1]
    chunks, found = _run(pre, start, n, lo_bit, [])
    if not found:
        return Plan(chunks, [], 1)
    nxt = np.append(np.flatnonzero(start), n)
    ov = [(s, int(nxt[np.searchsorted(nxt, s, side="right")])) for s in sorted(found)]
    chunks, again = _run(pre, start, n, lo_bit, ov)
    assert not again, "the second run found an unlisted big segment"
    return Plan(chunks, ov, 2)


# ---------------------------------------------------------------- the cases


@dataclass(frozen=True)
class Case:
    name: str
    family: str
    lo_bit: int
    key_bits: int
    segs: tuple
    why: str                    # the property the case is there for
    chunks: dict = field(default_factory=dict, hash=False, compare=False)  # tile -> {Chunk field: value}
    big: tuple = ()             # the big segments, (start, end)
    needs_sort: object = True   # the layout is not yet sorted (False: it is; None: either)
    rows: bool = True           # UNIQ emits a row, COUNT a group of 2 or more
    marks: tuple = ()           # (position in the sorted array, length) of groups that must be there

    @property
    def n(self):
        return sum(s.n for s in self.segs)

    @property
    def launches(self):
        return 2 if self.big else 1


@functools.lru_cache(maxsize=None)
def _keys(name):
    c = BY_NAME[name]
    keys = layout(c.segs, c.lo_bit, c.key_bits, np.random.default_rng(zlib.crc32(name.encode())))
    keys.setflags(write=False)
    return keys


def keys_of(case):
    """The case's keys (built once, read-only)."""
    return _keys(case.name)


def fill(total, big=300):
    """segment lengths adding up to total, none above `big`"""
    pat = (big, 1, 2, 37, 1, 150, 64, 3)
    out, i = [], 0
    while total > 0:
        out.append(min(pat[i % len(pat)], big, total))
        total -= out[-1]
        i += 1
    return out


def segs(lengths):
    """filler segments: distinct keys and pools of 3 in turn"""
    return tuple(Seg(n, "distinct" if i % 2 == 0 else ("pool", 3)) for i, n in enumerate(lengths))


def lens_with(total, marks):
    """group lengths adding up to total with a group of the given length
    heading at every marked position; between them groups of 1, 2, 1, 3, ..."""
    pat = (1, 2, 1, 3, 1, 1, 4)
    out, pos, i = [], 0, 0
    for head, ln in sorted(marks) + [(total, 0)]:
        assert head >= pos, "marks overlap"
        while pos < head:
            out.append(min(pat[i % len(pat)], head - pos))
            pos += out[-1]
            i += 1
        if ln:
            out.append(ln)
            pos += ln
    assert pos == total
    return tuple(out)


def _bits_for(nseg):
    return max(1, (nseg - 1).bit_length())


A_LENGTHS = (1, 2, 63, 64, 65, 127, 128, 129, W - 1, W, W + 1, 1023, 1024)
A_LOW = (1, 6, 7, 8, 14, 21, 22, 23, 28, 35, 50, 51, 52, 57, 63)


def _path_of(maxlen, low_bits):
    if maxlen <= W and low_bits <= WAVE_BITS:
        return "wave32" if low_bits <= U32_BITS else "wave64"
    return "block"


def _family_a():
    out = []
    for lb in A_LOW:
        room = 1 << min(64 - lb, 20)
        for length in A_LENGTHS:
            for draw in ("distinct", "pool"):
                def kind(n):
                    if draw == "pool":
                        return ("pool", min(3, 1 << lb))
                    return "distinct" if n <= (1 << lb) else ("pool", 1 << lb)
                short = [min(x, length) for x in (1, 2, 5, 40)]
                nfill = min(room - 1, 60)
                fl = [short[i % 4] for i in range(nfill)]
                lens = fl[:nfill // 2] + [length] + fl[nfill // 2:]
                tile = 0
                # the pool draw in the second of two chunks, where the prefix bits allow
                if draw == "pool" and room >= 8192:
                    lens = fill(C, max(1, min(length, 300))) + lens
                    tile = 1
                ss = tuple(Seg(n, kind(n)) for n in lens)
                want = {tile: dict(maxlen=length, path=_path_of(length, lb), first=0)}
                out.append(Case("A-lb%d-len%d-%s" % (lb, length, draw), "A%d" % lb, lb, lb + _bits_for(len(ss)), ss,
                                "maxlen == %d at %d low bits: %s" % (length, lb, want[tile]["path"]), want,
                                needs_sort=True if length >= 63 else None, rows=False))
    # no prefix at all: one segment, big once it cannot be staged
    for n in (W, 1024, R - 1, R, 2 * C + 7):
        big = ((0, n),) if n >= R else ()
        ch = {0: dict(tail="big", trail_pre=True, hi=C, path="block")} if big else \
            {0: dict(maxlen=n, path="block", hi=n, nsegs=1)}
        out.append(Case("A-lb64-n%d" % n, "A64", 64, 64, (Seg(n),), "lo_bit == key_bits == 64, %d keys: %s"
                        % (n, "big" if big else "block"), ch, big, rows=False))
    return out


def _family_b():
    out = []

    def eq(lengths):
        return tuple(Seg(n, "equal") for n in lengths)

    lens = [W, 1, 2, 100, 767, 64, 65, 1, 300] * 4  # 8256 keys: two chunks
    out.append(Case("B-wave", "B", 0, 12, eq(lens), "lo_bit == 0, every segment <= W: the wave path sorts nothing",
                    {0: dict(path="wave32", maxlen=W), 1: dict(path="wave32")}, needs_sort=False))
    lens = [300, 900, 1, 2, 500]
    out.append(Case("B-block", "B", 0, 12, eq(lens), "lo_bit == 0, a 900-key segment among others: block path",
                    {0: dict(path="block", maxlen=900)}, needs_sort=False))
    for n in (W + 1, 900, 1023):
        out.append(Case("B-block0-%d" % n, "B", 0, 4, eq([n]), "lo_bit == 0, one segment of %d: no pass at all" % n,
                        {0: dict(path="block0", maxlen=n, nsegs=1)}, needs_sort=False, rows=False))
    # a chunk whose owned range is one 800-key segment, after a segment that covers its head
    out.append(Case("B-block0-late", "B", 0, 4, eq([C + 10, 800]), "lo_bit == 0, chunk 1 owns one segment of 800",
                    {1: dict(path="block0", first=10, nsegs=1, maxlen=800)}, needs_sort=False, rows=False))
    # the only key is 0, the value a thread holds for "no neighbour": it is a head and a tail all the same
    out.append(Case("B-one-zero", "B", 0, 4, eq([1]), "one key, 0: a singleton whose neighbours are padding",
                    {0: dict(path="none", cnt=1)}, needs_sort=False, rows=False))
    out.append(Case("B-big", "B", 0, 12, eq([100, 1, 7000, 1, 50]), "lo_bit == 0, one big segment",
                    {0: dict(tail="big")}, ((101, 7101),), needs_sort=False))
    out.append(Case("B-ones", "B", 0, 13, eq([1] * C), "lo_bit == 0, a chunk of 1-key segments",
                    {0: dict(path="wave32", maxlen=1, nsegs=C)}, needs_sort=False, rows=False))
    return out


C_STARTS = (0, 1, 2500, C - 1)
C_ENDS = (C - 1, C, C + 1, L - 1, L, L + 1, R - 2, R - 1, R, R + 1)


def _family_c():
    out = []
    for s in C_STARTS:
        for e in C_ENDS:
            if e <= s:
                continue  # no such segment
            for follow in (True, False):
                lb = 20 if follow else 30
                head = fill(s)
                tgt = Seg(e - s, ("pool", 50) if (s + e) % 2 else "distinct")
                big = ((s, e),) if e >= R else ()
                if follow:
                    ss = segs(head) + (tgt, Seg(40), Seg(100, ("pool", 3)))
                    if e < C:  # the follower is the last owned segment
                        ch = dict(tail="loaded", hi=e + 40)
                    elif e < L:
                        ch = dict(tail="loaded", hi=e)
                    elif e < R:
                        ch = dict(tail="rounds", hi=e)
                    else:
                        ch = dict(tail="big", hi=C, trail_pre=True)
                else:
                    ss = segs(head) + (tgt,)
                    if e <= L:
                        ch = dict(tail="array_end", hi=e)
                    elif e < R:
                        ch = dict(tail="rounds", hi=e)
                    else:
                        ch = dict(tail="big", hi=C, trail_pre=True)
                name = "C-s%d-e%d-%s" % (s, e, "follow" if follow else "end")
                out.append(Case(name, "C%d" % s, lb, lb + 13, ss, "last owned segment [%d, %d): %s, hi == %d"
                                % (s, e, ch["tail"], ch["hi"]), {0: ch}, big, rows=s > 1 or follow))
    # the second chunk's last owned segment runs to the end of the array
    for d, tail in ((C + 1, "array_end"), (L, "array_end"), (L + 1, "rounds")):
        ss = segs(fill(2 * C - 10)) + (Seg(10 + d - C, ("pool", 9)),)
        out.append(Case("C-rest%d" % d, "Crest", 20, 33, ss, "n - base == %d in chunk 1: %s" % (d, tail),
                        {1: dict(tail=tail, hi=d), 2: dict(has_start=False, tail="none", path="none")}))
    return out


def _family_d():
    out = []

    def case(name, why, ss, big, chunks, **kw):
        out.append(Case("D-" + name, "D", 20, 33, tuple(ss), why, chunks, tuple(big), **kw))

    p50, tailf = ("pool", 50), segs(fill(500))
    case("index0", "a big segment at array index 0", (Seg(7000, p50),) + tailf, [(0, 7000)],
         {0: dict(tail="big", first=0), 1: dict(lead_pre=True, lo=0)})
    case("chunk-offset0", "a big segment at offset 0 of chunk 1", segs(fill(C)) + (Seg(7000),) + tailf,
         [(C, C + 7000)], {1: dict(tail="big", first=0, owned=1), 2: dict(lead_pre=True)})
    case("last-owned", "a big segment at offset C - 1", segs(fill(2 * C - 1)) + (Seg(2000, p50),) + tailf,
         [(2 * C - 1, 2 * C + 1999)], {1: dict(tail="big"), 2: dict(lead_pre=True, first=1999)})
    for e in (2 * C - 1, 2 * C, 2 * C + 1):
        ch = {0: dict(tail="big"), 1: dict(lead_pre=True)}
        if e == 2 * C - 1:
            ch[1].update(first=C - 1, has_start=True)
            ch[2] = dict(lead_pre=False)
        elif e == 2 * C:
            ch[1].update(has_start=False)
            ch[2] = dict(lead_pre=False, first=0)
        else:
            ch[1].update(has_start=False)
            ch[2] = dict(lead_pre=True, first=1)
        case("end%d" % e, "a big segment ending at %d (2C%+d)" % (e, e - 2 * C),
             segs(fill(3000)) + (Seg(e - 3000, p50),) + tailf, [(3000, e)], ch)
    case("to-n", "a big segment ending at n", segs(fill(1000)) + (Seg(8000, p50),), [(1000, 9000)],
         {0: dict(tail="big"), 1: dict(lead_pre=True, has_start=False, hi=9000 - C)})
    case("whole", "one big segment is the whole array", (Seg(12000, ("groups", lens_with(12000, ()))),), [(0, 12000)],
         {0: dict(tail="big", owned=1), 1: dict(lead_pre=True, has_start=False), 2: dict(lead_pre=True)})
    case("pair", "two big segments back to back", segs(fill(100)) + (Seg(7000, p50), Seg(7000)) + segs(fill(100)),
         [(100, 7100), (7100, 14100)], {0: dict(tail="big"), 1: dict(lead_pre=True, tail="big", first=1980)})
    case("cover", "a big segment covers chunks 1 and 2 whole", segs(fill(4000)) + (Seg(3 * C, p50),) + tailf,
         [(4000, 4000 + 3 * C)],
         {1: dict(lead_pre=True, has_start=False, lo=0, hi=C), 2: dict(lead_pre=True, has_start=False),
          3: dict(lead_pre=True, has_start=True, first=4000)})
    case("then-ones", "a big segment, then 1-key segments", (Seg(7000, p50),) + tuple(Seg(1) for _ in range(600)),
         [(0, 7000)], {1: dict(lead_pre=True, first=7000 - C, maxlen=7000 - C)})
    case("shortest", "the shortest big segment: R - C + 1 keys at offset C - 1",
         segs(fill(C - 1)) + (Seg(R - C + 1),) + tailf, [(C - 1, R)], {0: dict(tail="big", hi=C)})
    return out


GALLOP = (1, 2, 3, 4, 5, 8, 9, 16, 17)


def _family_e():
    out = []
    # one segment, the whole array: a group headed by the last key of chunk
    # j - 1 runs 1 .. 17 keys into chunk j; the first key a singleton; the last
    # group runs to n
    n = 10 * C + 300
    marks = [(0, 1)] + [(j * C - 1, 1 + k) for j, k in zip(range(1, 10), GALLOP)] + [(n - 40, 40)]
    out.append(Case("E-head-last", "E", 20, 21, (Seg(n, ("groups", lens_with(n, marks))),),
                    "groups headed by a chunk's last key, 1..17 keys into the next; a group running to n",
                    {0: dict(tail="big"), 9: dict(lead_pre=True, has_start=False)}, ((0, n),), marks=tuple(marks)))
    # a segment from 2000 to n: singletons on both sides of a chunk end, a
    # group over three chunks, heads 5 keys before a chunk end, a singleton last
    s, n = 2000, 9 * C + 100
    marks = [(C - 1, 1), (C, 1), (2 * C - 10, C + 20)] + \
        [(j * C - 5, 5 + k) for j, k in zip(range(4, 9), (1, 2, 4, 8, 16))] + [(n - 1, 1)]
    rel = [(p - s, ln) for p, ln in marks]
    out.append(Case("E-head-mid", "E", 20, 33, segs(fill(s)) + (Seg(n - s, ("groups", lens_with(n - s, rel))),),
                    "singletons across a chunk end, a group over three chunks, a singleton as the last key",
                    {0: dict(tail="big"), 2: dict(lead_pre=True, has_start=False)}, ((s, n),), marks=tuple(marks)))
    return out


def _family_f():
    out = []
    for n in (1, 2, C - 1, C, C + 1, 2 * C, 2 * C + 1):
        nch = (n + C - 1) // C
        ch = {nch - 1: dict(cnt=n - (nch - 1) * C)}
        if n == 1:
            ch[0].update(path="none")
        out.append(Case("F-n%d" % n, "F", 20, 33, segs(fill(n)), "n == %d: %d chunk(s)" % (n, nch), ch,
                        needs_sort=True if n > 2 else None, rows=n > 2))
    out.append(Case("F-ones", "F", 20, 33, tuple(Seg(1) for _ in range(C)), "a chunk of 5120 1-key segments",
                    {0: dict(nsegs=C, maxlen=1, path="wave32")}, needs_sort=False, rows=False))
    out.append(Case("F-alt", "F", 20, 33, tuple(Seg(1 + i % 2, "equal") for i in range(3600)),
                    "1- and 2-key segments in turn", {0: dict(maxlen=2, path="wave32"), 1: dict(maxlen=2)},
                    needs_sort=False))
    out.append(Case("F-segC", "F", 20, 33, (Seg(C, ("pool", 700)),) + segs(fill(400)),
                    "one segment of exactly C keys at offset 0",
                    {0: dict(first=0, hi=C, tail="loaded", maxlen=C, nsegs=1, path="block"), 1: dict(first=0)}))
    # groups over the 12-item boundaries of the run-length pass
    marks = ((11, 2), (23, 2), (35, 3), (46, 4))
    out.append(Case("F-rl12", "F", 20, 33, (Seg(600, ("groups", lens_with(600, marks))),) + segs(fill(300)),
                    "groups over positions 11-12, 23-24 (one thread's items end there)",
                    {0: dict(lo=0, path="wave32")}, marks=marks))
    marks = ((6131, 2), (6141, 2))
    rel = tuple((p - 5000, ln) for p, ln in marks)
    out.append(Case("F-rl-hi", "F", 20, 33,
                    segs(fill(5000)) + (Seg(R - 1 - 5000, ("groups", lens_with(R - 1 - 5000, rel))), Seg(50)),
                    "hi == R - 1: groups over 6131-6132 and up to the last staged position",
                    {0: dict(lo=0, hi=R - 1, tail="rounds", path="block")}, marks=marks))
    return out


CASES = _family_a() + _family_b() + _family_c() + _family_d() + _family_e() + _family_f()
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)
FAMILIES = sorted({c.family for c in CASES}, key=lambda f: (f[0], int(f[1:]) if f[1:].isdigit() else -1))


def family(name):
    return [c for c in CASES if c.family == name]
