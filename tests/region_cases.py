"""The capacity contract of the region path (kman_groups), restated on the
CPU, and inputs that fill one region to exactly a chosen size.

numpy and Python only (importable without a GPU): tests/test_region_cases_cpu.py
proves the restatement against kman_groups_plan and every builder against
np_oracle; tests/test_gpu_region_edges.py runs the inputs on the device.

Geometry (region_extract.hip, region_pass.hip, region_finish.hip):

* pass 0: a window belongs to the tile of its start, tile = p // (512 * ei)
  (ei = 16, or 8 with -r: then a window's two items share its tile).  kman_groups
  interleaves the tiles over the 64 position segments, s = tile % 64 (the
  contiguous layout, tile // seg_tiles, is the multi-GPU shard path's), so
  segment s holds the tiles s, s + 64, s + 128, ...  Region (b, s) takes the
  items of bucket b (the top 8 key bits) of those tiles, at most C0.
* pass 1: bucket b's items are one stream, segment after segment, cut into
  pass tiles of 8192 items; chain 0 takes the first ceil(tiles / 2) pass
  tiles, chain 1 the rest.  A bucket of at most 8192 items is all chain 0.
  Sub-region (r, h) takes the items of region r (the top 8 + B2 key bits)
  that chain h reads, at most C1.  Items inside a region (b, s) are in no
  fixed order, so where the cut falls inside a segment only bounds are known:
  fills() returns both; they agree when the cut is at a segment boundary.
* finish: region r is its two sub-regions, m0 + m1 <= FCAP items.
"""

from __future__ import annotations

import functools
from dataclasses import dataclass

import numpy as np

import np_oracle

RT, RS, G1, H = 512, 64, 8, 2
FCAP, FFILL_T, FFILL_M = 8704, 6144, 7800
PASS_TILE = 8192  # items per pass-1 tile (1024 threads x 8)
KMAN_OK, KMAN_EINVAL, KMAN_EFALLBACK = 0, -1, -8
FLAG_RC, FLAG_WANT_POS, FLAG_CANONICAL = 1, 2, 4
MODE_COUNT, MODE_UNIQ = 1, 2


def _ceil_div(a: int, b: int) -> int:
    return -(-a // b)


@dataclass(frozen=True)
class Plan:
    verdict: int
    K: int = 0
    W: int = 0
    Q: int = 0
    B2: int = 0
    rest: int = 0
    C0: int = 0
    C1: int = 0  # (C1h: the capacity of each of the H sub-regions)
    H: int = H
    ei: int = 0
    tile: int = 0  # windows per pass-0 tile
    n_tiles0: int = 0
    # (as make_plan records it; kman_groups itself never reads it -- its
    # segments are interleaved, s = tile % 64 -- only the shard path does)
    seg_tiles: int = 0
    nreg: int = 0
    work_bytes: int = 0


def plan(n_bases: int, k: int, rc: bool = False, mode="count", canonical: bool = False) -> Plan:
    """make_plan of region_groups.hip.  mode: "count" / "uniq" or the ABI's
    integer (anything else: KMAN_EINVAL)."""
    mode = {"count": MODE_COUNT, "uniq": MODE_UNIQ}.get(mode, mode)
    if mode not in (MODE_COUNT, MODE_UNIQ) or k < 2 or k > 32:
        return Plan(KMAN_EINVAL)
    uniq = mode == MODE_UNIQ
    if (uniq and k > 25) or n_bases == 0:
        return Plan(KMAN_EFALLBACK)
    rc = rc and not canonical
    K = 2 * k
    W = n_bases * (2 if rc else 1)
    Q = max(1, int(W - 1).bit_length()) if uniq else 0
    if K - G1 + Q > 64:
        return Plan(KMAN_EFALLBACK)
    b2 = 1
    while b2 < 9 and (W >> (G1 + b2)) > FFILL_T and (G1 + b2 < 17 or (W >> (G1 + b2)) > FFILL_M):
        b2 += 1
    if (W >> (G1 + b2)) > FFILL_M or K < G1 + b2 + 1:
        return Plan(KMAN_EFALLBACK)
    ei = 8 if rc else 16
    n_tiles0 = _ceil_div(n_bases, RT * ei)
    e0 = W // ((1 << G1) * RS)
    C0 = _ceil_div(e0 + e0 // 2 + 256, 64) * 64
    if (1 << G1) * RS * C0 >= 1 << 32:
        return Plan(KMAN_EFALLBACK)
    e1 = W >> (G1 + b2)
    C1 = min(_ceil_div(e1 + e1 // 2 + 512, 64) * 64, FCAP)
    nreg = 1 << (G1 + b2)
    work = 256 * 64 * C0 * 8 + nreg * H * C1 * 8 + 256 * 64 * 4 + nreg * H * 4 + 64
    return Plan(KMAN_OK, K, W, Q, b2, K - G1 - b2, C0, C1, H, ei, RT * ei, n_tiles0, _ceil_div(n_tiles0, RS), nreg,
                work)


@dataclass(frozen=True)
class Fills:
    r0: np.ndarray      # [256, 64] items of pass-0 region (b, s)
    sub_lo: np.ndarray  # [nreg, 2] fewest items sub-region (r, h) can get
    sub_hi: np.ndarray  # [nreg, 2] most
    fin: np.ndarray     # [nreg] items of finish region r


def fills(keys: np.ndarray, pos: np.ndarray, pl: Plan) -> Fills:
    """Item counts of every region for the oracle's k-mer stream
    (np_oracle.stream_kmers: pos = window start << 1 | strand)."""
    nb = 1 << G1
    seg = ((pos >> np.uint64(1)) // np.uint64(pl.tile) % np.uint64(RS)).astype(np.int64)
    reg = (keys >> np.uint64(pl.rest)).astype(np.int64)
    rs = np.bincount(reg * RS + seg, minlength=pl.nreg * RS).reshape(pl.nreg, RS)
    r0 = rs.reshape(nb, 1 << pl.B2, RS).sum(axis=1)
    fin = rs.sum(axis=1)
    # the bucket's stream as pass 1 reads it (a cursor past C0 reads as C0;
    # such a call falls back whatever pass 1 does)
    c = np.minimum(r0, pl.C0)
    end = np.cumsum(c, axis=1)
    pre = end - c
    items = end[:, -1]
    tiles = -(-items // PASS_TILE)
    cut = np.minimum(-(-tiles // H) * PASS_TILE, items)[:, None]
    whole = end <= cut
    part = (pre < cut) & ~whole
    need = np.where(part, cut - pre, 0)
    d = 1 << pl.B2
    whole_r, part_r = np.repeat(whole, d, axis=0), np.repeat(part, d, axis=0)
    need_r, c_r = np.repeat(need, d, axis=0), np.repeat(c, d, axis=0)
    base = (rs * whole_r).sum(axis=1)
    lo0 = base + (np.maximum(0, need_r - (c_r - rs)) * part_r).sum(axis=1)
    hi0 = base + (np.minimum(need_r, rs) * part_r).sum(axis=1)
    sub_lo = np.stack([lo0, fin - hi0], axis=1)
    sub_hi = np.stack([hi0, fin - lo0], axis=1)
    return Fills(r0, sub_lo, sub_hi, fin)


# ------------------------------------------------------------------ builders
# The target is always bucket 0 (keys that start AAAA) and, of its two
# regions (every builder's plan has B2 = 1), region 0: a fifth base of A or C
# ("d0" below; G or T is region 1, "d1").  Filler goes into chosen tiles:
# one run of A (the repeated key AAA...A and, at its end, a few distinct
# keys) and blocks AAAAC + tail / AAAA[GT] + tail with random tails of C, G
# and T (distinct keys of region 0 / region 1; a block adds exactly one item).  Every count is taken from
# np_oracle's stream, so -r, canonical keys and other k need no special case.

_ASCII = np.frombuffer(b"ACGT", dtype=np.uint8)
_MARGIN = 64  # filler starts this far into its tile and ends as far before its end


def _stream(codes: np.ndarray, k: int, rc: bool, canonical: bool):
    return np_oracle.stream_kmers([(b"", _ASCII[codes].tobytes())], k, rc=rc, canonical=canonical)


def _tile_d(codes, t, pl, k, rc, canonical):
    """(d0, d1) items of the windows that start in pass-0 tile t."""
    lo = t * pl.tile
    hi = min(lo + pl.tile, len(codes) - k + 1)
    if not rc and not canonical:
        # forward keys: the top 9 bits are the window's first five bases (the
        # finished input is still counted from np_oracle's stream, in build())
        w = codes[lo:hi + 4]
        b0 = (w[:-4] == 0) & (w[1:-3] == 0) & (w[2:-2] == 0) & (w[3:-1] == 0)
        d0 = int((b0 & (w[4:] < 2)).sum())
        return d0, int(b0.sum()) - d0
    keys, _ = _stream(codes[lo:hi + k - 1], k, rc, canonical)
    top = keys >> np.uint64(pl.rest)
    return int((top == 0).sum()), int((top == 1).sum())


def _filler(a, c, g, tails, pad=1):
    tl = tails.shape[1]
    parts = [np.array([1], np.uint8)]
    if a > 0:  # (closed by C: the run's last AAAA is a region-0 item too, not a region-1 item)
        parts.append(np.zeros(a + 4, np.uint8))
        parts.append(np.array([1], np.uint8))
    parts.append(np.array([2], np.uint8))
    for i in range(c + g):
        parts.append(np.array([0, 0, 0, 0, 1 if i < c else 2 + (i & 1)], np.uint8))
        parts.append(tails[i, :tl])
    parts.append(np.full(pad, 2, np.uint8))
    return np.concatenate(parts)


def _set_tile(codes, t, want0, want1, pl, k, rc, canonical, rng, tail, margin=_MARGIN):
    """Rewrite the filler of tile t until the tile has exactly want0 region-0
    items and (unless None) want1 region-1 items."""
    lo = t * pl.tile
    assert lo + pl.tile <= len(codes) - k, "filler only in whole tiles"
    pristine = codes[lo:lo + pl.tile].copy()
    tails = rng.integers(1, 4, size=(pl.C0 + 8, tail)).astype(np.uint8)
    b0, b1 = _tile_d(codes, t, pl, k, rc, canonical)
    add0, add1 = want0 - b0, (0 if want1 is None else want1 - b1)
    if add0 == 0 and add1 == 0:
        return
    assert add0 >= 0 and add1 >= 0, "the background already exceeds the wanted fill"
    # the run of A carries most of region 0's filler: a block also puts its
    # shifted windows into a few other regions (AAAC., .AAAA), a run does not.
    # With -r every run item is also a TTT...T item of bucket 255: half blocks
    c = add0 if add0 < 8 else (add0 // 2 if rc else min(add0 // 2, 4))
    a, g = add0 - c, add1
    pad = 1
    for it in range(48):
        # (a step can go over the target -- a block whose tail adds an item of
        # its own, a background item at the filler's end that one more base
        # covers: other tails, another end)
        if it % 4 == 3:
            tails = rng.integers(1, 4, size=tails.shape).astype(np.uint8)
            pad = int(rng.integers(1, 9))
        f = _filler(a, c, g, tails, pad)
        assert margin + len(f) + _MARGIN <= pl.tile, "filler does not fit its tile"
        codes[lo:lo + pl.tile] = pristine
        codes[lo + margin:lo + margin + len(f)] = f
        m0, m1 = _tile_d(codes, t, pl, k, rc, canonical)
        if m0 == want0 and (want1 is None or m1 == want1):
            return
        # (a run of a + 4 A and its closing C: a + 1 items; a block: one)
        diff = want0 - m0
        if a > 0 and a + diff >= 1:
            a += diff
        else:
            c, a = c + diff + (a + 1 if a > 0 else 0), 0
        if want1 is not None:
            g += want1 - m1
        assert c >= 0 and g >= 0, "filler cannot reach the wanted fill"
    raise AssertionError("filler did not converge")


def _seg_tiles(pl, s):
    # (never the stream's last tile: it may be short)
    return [t for t in range(s, pl.n_tiles0 - 1, RS)]


def _set_segment(codes, s, want0, want1, pl, k, rc, canonical, rng, tail, only=None):
    """Spread filler over the tiles of segment s (or only these of them)
    until they have exactly want0 region-0 and (unless None) want1 region-1
    items."""
    ts = _seg_tiles(pl, s) if only is None else list(only)
    every = list(range(s, pl.n_tiles0, RS)) if only is None else list(only)
    cur = {t: _tile_d(codes, t, pl, k, rc, canonical) for t in every}
    add0 = want0 - sum(v[0] for v in cur.values())
    add1 = None if want1 is None else want1 - sum(v[1] for v in cur.values())
    for i, t in enumerate(ts):
        left = len(ts) - i
        s0 = add0 // left
        s1 = None if add1 is None else add1 // left
        _set_tile(codes, t, cur[t][0] + s0, None if s1 is None else cur[t][1] + s1, pl, k, rc, canonical, rng, tail)
        add0 -= s0
        if add1 is not None:
            add1 -= s1


def _seg_d(codes, s, pl, k, rc, canonical):
    d = [_tile_d(codes, t, pl, k, rc, canonical) for t in range(s, pl.n_tiles0, RS)]
    return sum(v[0] for v in d), sum(v[1] for v in d)


def _scrub_d0(codes, tiles, pl):
    """No forward window that starts in these tiles stays in region 0: the
    fifth base of AAAAA / AAAAC becomes G (region 1)."""
    for t in tiles:
        lo, hi = t * pl.tile, min((t + 1) * pl.tile, len(codes) - 4)
        while True:
            w = codes[lo:hi + 4]
            hit = (w[:-4] == 0) & (w[1:-3] == 0) & (w[2:-2] == 0) & (w[3:-1] == 0) & (w[4:] < 2)
            idx = np.nonzero(hit)[0]
            if not len(idx):
                break
            codes[lo + idx[0] + 4] = 2


def _scrub_bucket0(codes, t, pl):
    """No forward window that starts in tile t stays in bucket 0: the fourth
    base of AAAA becomes C."""
    lo, hi = t * pl.tile, min((t + 1) * pl.tile, len(codes) - 3)
    while True:
        w = codes[lo:hi + 3]
        idx = np.nonzero((w[:-3] == 0) & (w[1:-2] == 0) & (w[2:-1] == 0) & (w[3:] == 0))[0]
        if not len(idx):
            break
        codes[lo + idx[0] + 3] = 1


def _split(total, parts):
    return [total // parts + (1 if i < total % parts else 0) for i in range(parts)]


@dataclass(frozen=True)
class Case:
    text: bytes
    k: int
    rc: bool
    canonical: bool
    plan: Plan
    fills: Fills
    cap: int       # the capacity under test
    fill: int      # the target's fill: cap - 1, cap or cap + 1
    # every region meant to reach its stated fill: (kind, index, fill), kind
    # "r0" (index (b, s)), "sub" ((r, h)) or "fin" (r); all others stay
    # strictly below their capacities
    targets: tuple
    tiles: tuple   # the pass-0 tiles of the target segment (the C0 edges)
    tile_fills: tuple  # the bucket-0 items each of them brings


EDGES = ("c0_tile", "c0_seg3", "c1_chain0", "c1_chain1", "fin_both", "fin_m0")
# c0_late: c0_seg3 with the fill in the segment's first two tiles and the
# item over the capacity alone in its third -- in stream order (the
# three-call form) that tile finds the region's cursor at exactly C0
LATE = "c0_late"
EDGE_BASES = {"c0_tile": 400_000, "c0_seg3": 1_500_000, "c1_chain0": 400_000, "c1_chain1": 1_500_000,
              "fin_both": 1_500_000, "fin_m0": 2_800_000, LATE: 1_500_000}


def _aligned_chains(codes, pl, k, rc, canonical, rng, tail, n_front, front0, front_items, back0):
    """Bucket 0 with its chain cut on a segment boundary: the segments below
    n_front hold front_items items in all (a whole number of pass tiles: chain
    0 reads exactly these), front0 of them in region 0; the segments from
    n_front on (chain 1) hold back0 region-0 items, or stay as they are
    (back0 None)."""
    for s, w0, w in zip(range(n_front), _split(front0, n_front), _split(front_items, n_front)):
        _set_segment(codes, s, w0, w - w0, pl, k, rc, canonical, rng, tail)
    if back0 is not None:
        n_back = RS - n_front
        for s, w0 in zip(range(n_front, RS), _split(back0, n_back)):
            _set_segment(codes, s, w0, None, pl, k, rc, canonical, rng, tail)


@functools.lru_cache(maxsize=None)
def build(edge: str, delta: int, k: int = 21, rc: bool = False, canonical: bool = False) -> Case:
    """A single-record ACGT FASTA whose target region holds cap + delta items."""
    assert edge in EDGES + (LATE,) and delta in (-1, 0, 1)
    n = EDGE_BASES[edge]
    pl = plan(n, k, rc, "count", canonical)
    assert pl.verdict == KMAN_OK and pl.B2 == 1
    rng = np.random.default_rng([(EDGES + (LATE,)).index(edge), delta + 1, k, int(rc), int(canonical)])
    codes = rng.integers(0, 4, size=n).astype(np.uint8)
    tail = 3 if rc else 7
    args = (pl, k, rc, canonical, rng, tail)
    tiles = ()
    if edge in ("c0_tile", "c0_seg3"):
        # region (0, s) of pass 0: one tile (with -r the segment's second
        # tile keeps its background), or spread over the segment's three
        s = 20 if edge == "c0_tile" else 10
        cap = pl.C0
        tiles = tuple(range(s, pl.n_tiles0, RS))
        assert len(tiles) == (3 if edge == "c0_seg3" else (2 if rc else 1))
        cur0, cur1 = _seg_d(codes, s, *args[:4])
        want1 = cur1 + 2 * len(tiles)
        if edge == "c0_tile":
            t = tiles[0]
            t0, t1 = _tile_d(codes, t, *args[:4])
            # -r: a window that ends in the filler's AAAA is a TTTT... item of
            # bucket 255, in the tile of its start -- for the run's first k - 4
            # windows the tile before when the run starts with this one, which
            # keeps region (255, s) below the fill of (0, s)
            _set_tile(codes, t, t0 + (cap + delta - want1 - cur0), t1 + want1 - cur1, *args, margin=0 if rc else _MARGIN)
        else:
            _set_segment(codes, s, cap + delta - want1, want1, *args)
        targets = (("r0", (0, s), cap + delta),)
    elif edge == LATE:
        assert not rc and not canonical, "the scrub reads forward keys"
        s, cap = 10, pl.C0
        tiles = tuple(range(s, pl.n_tiles0, RS))
        assert len(tiles) == 3
        _scrub_bucket0(codes, tiles[2], pl)
        cur1 = sum(_tile_d(codes, t, *args[:4])[1] for t in tiles[:2])
        front = cap + min(delta, 0)
        _set_segment(codes, s, front - cur1 - 4, cur1 + 4, *args, only=tiles[:2])
        if delta > 0:
            _set_tile(codes, tiles[2], delta, 0, *args)
        targets = (("r0", (0, s), cap + delta),)
    elif edge == "c1_chain0":
        # a bucket of at most one pass tile: chain 0 reads all of it
        cap = pl.C1
        keys, pos = _stream(codes, k, rc, canonical)
        have = int(fills(keys, pos, pl).fin[0])
        need = cap + delta - have
        segs = list(range(4, 4 + _ceil_div(need, 100)))
        for s, w in zip(segs, _split(need, len(segs))):
            cur0, _ = _seg_d(codes, s, *args[:4])
            _set_segment(codes, s, cur0 + w, None, *args)
        targets = (("sub", (0, 0), cap + delta), ("fin", 0, cap + delta))
    elif edge == "c1_chain1":
        # chain 0 reads one pass tile (segments 0-31), chain 1 the rest
        cap = pl.C1
        m0 = 3500
        _aligned_chains(codes, *args, 32, m0, PASS_TILE, cap + delta)
        targets = (("sub", (0, 0), m0), ("sub", (0, 1), cap + delta), ("fin", 0, m0 + cap + delta))
    elif edge == "fin_both":
        cap = FCAP
        m0 = 4400
        _aligned_chains(codes, *args, 32, m0, PASS_TILE, cap + delta - m0)
        targets = (("sub", (0, 0), m0), ("sub", (0, 1), cap + delta - m0), ("fin", 0, cap + delta))
    else:
        # C1 = FCAP: chain 0 (two pass tiles, segments 0-55) alone fills the
        # region; chain 1 adds nothing, or one item
        assert not rc and not canonical, "the scrub reads forward keys"
        cap = FCAP
        assert pl.C1 == FCAP
        m0, m1 = cap + min(delta, 0), max(delta, 0)
        _scrub_d0(codes, [t for t in range(pl.n_tiles0) if t % RS >= 56], pl)
        _aligned_chains(codes, *args, 56, m0, 2 * PASS_TILE, None)
        if m1:
            _set_segment(codes, 60, m1, None, *args)
        targets = (("sub", (0, 0), m0), ("sub", (0, 1), m1), ("fin", 0, cap + delta))
    keys, pos = _stream(codes, k, rc, canonical)
    b0 = (pos >> np.uint64(1))[(keys >> np.uint64(pl.K - G1)) == 0] // np.uint64(pl.tile)
    tile_fills = tuple(int((b0 == t).sum()) for t in tiles)
    return Case(b">edge\n" + _ASCII[codes].tobytes() + b"\n", k, rc, canonical, pl, fills(keys, pos, pl), cap,
                cap + delta, targets, tiles, tile_fills)


# -r: what the filler's reverse strand puts into the last bucket, recorded
# from np_oracle's stream: (edge, delta) -> (region (255, s) of the target's
# segment, finish regions 510 and 511)
RC_FILLS = {("c0_tile", -1): (367, 1694, 1841), ("c0_tile", 0): (368, 1664, 1794), ("c0_tile", 1): (367, 1722, 1848),
            ("c1_chain0", -1): (72, 2039, 2453), ("c1_chain0", 0): (56, 2000, 2479),
            ("c1_chain0", 1): (76, 2011, 2470)}


def rc_fills(case: Case):
    f = case.fills
    return int(f.r0[255, 20]), int(f.fin[-2]), int(f.fin[-1])


def capacity_report(case: Case):
    """-> (targets as found, the fullest non-target region of each kind as a
    fraction-free pair (fill, capacity))."""
    f, pl = case.fills, case.plan
    found = []
    r0, hi, fin = f.r0.copy(), f.sub_hi.copy(), f.fin.copy()
    for kind, idx, _ in case.targets:
        if kind == "r0":
            found.append(int(f.r0[idx]))
            r0[idx] = -1
        elif kind == "sub":
            found.append((int(f.sub_lo[idx]), int(f.sub_hi[idx])))
            hi[idx] = -1
        else:
            found.append(int(f.fin[idx]))
            fin[idx] = -1
    return found, ((int(r0.max()), pl.C0), (int(hi.max()), pl.C1), (int(fin.max()), FCAP))
