"""CPU checks of tests/finish_cases.py: every layout of the table is what
tests/test_gpu_finish_edges.py says it is.  plan() -- the restatement of
segfin_kernel's per-chunk decisions (kman_amd/csrc/segsort.hip) -- reports
for each entry exactly the property the entry names; the layout is sorted by
prefix and, where a sort is the point, not by key; np_oracle's answer has the
rows the property needs.  No entry is skipped anywhere: a case added with the
wrong property fails here.  kman_split_bits, a pure host function, is pinned
at every 512 * 2^p boundary (the library loads without a GPU)."""

from __future__ import annotations

from ctypes import byref, c_uint32

import numpy as np
import pytest

import finish_cases as F


def test_the_constants_are_the_kernels():
    """C, R, L, W and the two bit limits as segsort.hip spells them."""
    import os
    import re

    src = open(os.path.join(os.path.dirname(__file__), "..", "kman_amd", "csrc", "segsort.hip")).read()

    def const(name):
        return int(re.search(r"constexpr int %s = (\d+);" % name, src).group(1))

    assert (const("FT"), const("FC"), const("FR"), const("WI") * 64) == (F.FT, F.C, F.R, F.W)
    assert "constexpr int PI = FC / FT + 1;" in src and F.L == (F.C // F.FT + 1) * F.FT
    assert "maxlen <= (uint32_t)(WI * 64) && low_bits <= %d" % F.WAVE_BITS in src
    assert "if (low_bits <= %d)" % F.U32_BITS in src
    assert "for (uint32_t r0 = PI * FT; r0 < (uint32_t)FR; r0 += FT)" in src


def test_layout_refuses_what_does_not_fit():
    rng = np.random.default_rng(1)
    with pytest.raises(ValueError):
        F.layout([F.Seg(1)] * 5, 10, 12, rng)  # 5 segments, 4 prefixes
    with pytest.raises(ValueError):
        F.layout([F.Seg(3)], 1, 4, rng)  # 3 distinct values of one bit
    with pytest.raises(ValueError):
        F.layout([F.Seg(2)], 0, 4, rng)  # lo_bit == 0: a segment is one group
    with pytest.raises(ValueError):
        F.layout([F.Seg(5, ("groups", (2, 2)))], 8, 12, rng)
    with pytest.raises(ValueError):
        F.layout([F.Seg(1)], 13, 12, rng)
    keys = F.layout([F.Seg(4)] * 4, 10, 12, rng)
    assert (keys >> np.uint64(10)).tolist() == [0] * 4 + [1] * 4 + [2] * 4 + [3] * 4 and keys.max() < 1 << 12


def test_the_table_covers_what_it_claims():
    names = set(F.BY_NAME)
    assert len(F.CASES) == len(names)
    for lb in F.A_LOW:
        for ln in F.A_LENGTHS:
            assert {"A-lb%d-len%d-distinct" % (lb, ln), "A-lb%d-len%d-pool" % (lb, ln)} <= names
    assert F.A_LENGTHS == (1, 2, 63, 64, 65, 127, 128, 129, 767, 768, 769, 1023, 1024)
    assert F.A_LOW == (1, 6, 7, 8, 14, 21, 22, 23, 28, 35, 50, 51, 52, 57, 63)
    assert F.C_STARTS == (0, 1, 2500, 5119)
    assert F.C_ENDS == (5119, 5120, 5121, 5631, 5632, 5633, 6142, 6143, 6144, 6145)
    for s in F.C_STARTS:
        for e in F.C_ENDS:
            if e > s:
                assert {"C-s%d-e%d-follow" % (s, e), "C-s%d-e%d-end" % (s, e)} <= names
    paths = {ch["path"] for c in F.CASES for ch in c.chunks.values() if "path" in ch}
    tails = {ch["tail"] for c in F.CASES for ch in c.chunks.values() if "tail" in ch}
    assert paths == {"none", "wave32", "wave64", "block", "block0"}
    assert tails == {"none", "loaded", "array_end", "rounds", "big"}
    assert F.keys_of(F.BY_NAME["B-one-zero"]).tolist() == [0]
    assert max(c.n for c in F.CASES) < 60_000
    assert {c.family[0] for c in F.CASES} == set("ABCDEF")


@pytest.mark.parametrize("fam", F.FAMILIES)
def test_every_entry_has_its_property(fam):
    import np_oracle

    cases = F.family(fam)
    assert cases
    for c in cases:
        keys = F.keys_of(c)
        assert len(keys) == c.n and c.why
        if c.key_bits < 64:
            assert int(keys.max()) < 1 << c.key_bits, c.name
        pre = F.prefixes(keys, c.lo_bit)
        assert (pre[1:] >= pre[:-1]).all(), c.name
        want_k, want_v = np_oracle.stable_sort(keys, np.arange(c.n, dtype=np.uint64))
        if c.needs_sort:
            assert not np.array_equal(keys, want_k), "%s: already sorted" % c.name
        elif c.needs_sort is False:
            assert np.array_equal(want_v, np.arange(c.n, dtype=np.uint64)), c.name
        pl = F.plan(keys, c.lo_bit)
        assert pl.launches == c.launches and tuple(pl.big) == tuple(c.big), (c.name, pl.big)
        assert c.chunks, c.name
        for tile, want in c.chunks.items():
            got = {f: getattr(pl.chunks[tile], f) for f in want}
            assert got == want, (c.name, tile, pl.chunks[tile])
        for s, e in c.big:  # a big segment is one no chunk could stage: it ends at offset R or beyond
            assert s % F.C + (e - s) >= F.R and pre[s] == pre[e - 1] and (e == c.n or pre[e] != pre[s])
            assert s == 0 or pre[s - 1] != pre[s]
        ck, cc = np_oracle.rle_count(want_k)
        uk, uv = np_oracle.rle_uniq(want_k, want_v)
        assert int(cc.sum()) == c.n and len(uk) == int((cc == 1).sum())
        if c.rows:
            assert len(uk) > 0 and int(cc.max()) > 1, c.name
        for pos, ln in c.marks:  # a group of exactly ln keys heads at sorted position pos
            assert (want_k[pos:pos + ln] == want_k[pos]).all(), (c.name, pos)
            assert pos == 0 or want_k[pos - 1] != want_k[pos], (c.name, pos)
            assert pos + ln == c.n or want_k[pos + ln] != want_k[pos], (c.name, pos)


def test_the_staging_rule_at_its_edge():
    """The last owned segment is staged up to an end at offset R - 1 and big
    from R on, wherever it starts; at offset C - 1 that is 1024 against 1025
    keys."""
    rng = np.random.default_rng(5)
    for s in (0, 1, 2500, F.C - 1):
        for e, big in ((F.R - 1, False), (F.R, True)):
            for rest in ((), (F.Seg(9),)):
                keys = F.layout(F.segs(F.fill(s)) + (F.Seg(e - s),) + rest, 20, 33, rng)
                pl = F.plan(keys, 20)
                assert (pl.launches, pl.big) == ((2, [(s, e)]) if big else (1, [])), (s, e)
    assert F.R - (F.C - 1) == 1025


# ---------------------------------------------------------------- kman_split_bits


def _want_split(n, key_bits):
    """the largest lo_bit with n >> (key_bits - lo_bit) <= 512, 0 if none"""
    for lo in range(key_bits, -1, -1):
        if n >> (key_bits - lo) <= 512:
            return lo
    return 0


@pytest.mark.parametrize("key_bits", [1, 4, 6, 8, 42, 64])
def test_split_bits_at_every_boundary(key_bits):
    from kman_amd import _native as N
    from kman_amd import engine

    L = N.lib()
    lo = c_uint32(99)
    seen = set()
    ns = {0, 1, 511, 512, 513, 2**64 - 1}
    for p in range(0, 55):
        ns |= {(512 << p) - 1, 512 << p, (512 << p) + 1}
    for n in sorted(ns):
        assert L.kman_split_bits(n, key_bits, byref(lo)) == N.KMAN_OK
        assert lo.value == _want_split(n, key_bits), (n, key_bits)
        assert 0 <= lo.value <= key_bits
        if n < 2**63:
            assert engine.split_bits(n, key_bits) == lo.value
        seen.add(lo.value)
    # it bottoms out at 0: from one key past 512 * 2^key_bits on
    assert max(seen) == key_bits
    if key_bits <= 42:
        for n in ((512 << key_bits) + 1, 4 * (512 << key_bits), 2**64 - 1):
            assert L.kman_split_bits(n, key_bits, byref(lo)) == N.KMAN_OK and lo.value == 0
    else:
        assert min(seen) == key_bits - 55  # (2^64 - 1) >> 55 == 511


def test_split_bits_refusals_and_the_engine_case():
    from kman_amd import _native as N
    from kman_amd import engine

    L = N.lib()
    lo = c_uint32(99)
    for kb in (0, 65, 1000):
        assert L.kman_split_bits(1000, kb, byref(lo)) == N.KMAN_EINVAL
        assert lo.value == 99
        with pytest.raises(ValueError):
            engine.split_bits(1000, kb)
    assert L.kman_split_bits(1000, 8, None) == N.KMAN_EINVAL
    # the sizes at which engine.sort reaches kman_finish with lo_bit == 0
    assert engine.split_bits(40_000, 6) == 0 and engine.split_bits(32_769, 6) == 0
    assert engine.split_bits(131_073, 8) == 0
    # (0 from 513 * 2^(key_bits - 1) keys on)
    assert engine.split_bits(513 * 32 - 1, 6) == 1 and engine.split_bits(513 * 32, 6) == 0
