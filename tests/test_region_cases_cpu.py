"""CPU checks of tests/region_cases.py: the plan restatement equals
kman_groups_plan (the library loads without a GPU), and np_oracle's stream
proves every built input is what tests/test_gpu_region_edges.py says it is --
the target regions at exactly their stated fills, every other region strictly
inside all three capacities."""

from __future__ import annotations

from ctypes import byref, c_uint64

import numpy as np
import pytest

import region_cases as R


def _sizes():
    s = {1, 2, 3, 20, 21, 25, 31, 32, 33, 1000, 400_000, 800_000, 1_500_000, 2_796_543, 2_796_544, 2_800_000,
         3_145_727, 3_145_728, 3_145_729, 10**9, 2 * 10**9, 3 * 10**9}
    for e in range(4, 32):
        s |= {(1 << e) - 1, 1 << e, (1 << e) + 1}
    # where FFILL_T / FFILL_M decide the region bits and the fallback
    for b in range(9, 18):
        for f in (R.FFILL_T, R.FFILL_M):
            s |= {(f << b) - 1, f << b, (f + 1) << b, ((f + 1) << b) + 1}
    return sorted(x for x in s if 1 <= x <= 3 * 10**9)


def test_plan_equals_kman_groups_plan(monkeypatch):
    from kman_amd import _native as N

    monkeypatch.delenv("KMAN_NO_REGION", raising=False)
    assert (R.KMAN_OK, R.KMAN_EINVAL, R.KMAN_EFALLBACK) == (N.KMAN_OK, N.KMAN_EINVAL, N.KMAN_EFALLBACK)
    assert (R.FLAG_RC, R.FLAG_WANT_POS, R.FLAG_CANONICAL) == (N.KMAN_RC, N.KMAN_WANT_POS, N.KMAN_CANONICAL)
    assert (R.MODE_COUNT, R.MODE_UNIQ) == (N.KMAN_FINISH_COUNT, N.KMAN_FINISH_UNIQ)
    L = N.lib()
    wb = c_uint64(0)
    seen = set()
    for n in [0] + _sizes():
        for k in (5, 9, 13, 21, 25, 31, 32):
            for rc in (False, True):
                for canonical in (False, True):
                    for mode in (N.KMAN_FINISH_COUNT, N.KMAN_FINISH_UNIQ):
                        flags = (N.KMAN_RC if rc else 0) | (N.KMAN_CANONICAL if canonical else 0) | \
                            (N.KMAN_WANT_POS if mode == N.KMAN_FINISH_UNIQ else 0)
                        got = L.kman_groups_plan(n, k, flags, mode, byref(wb))
                        pl = R.plan(n, k, rc, mode, canonical)
                        assert (got, wb.value) == (pl.verdict, pl.work_bytes), (n, k, rc, canonical, mode)
                        seen.add(got)
    assert seen == {N.KMAN_OK, N.KMAN_EFALLBACK}
    for n, k, mode in ((1000, 21, N.KMAN_FINISH_SORT), (1000, 21, 3), (1000, 1, 1), (1000, 33, 1), (0, 33, 2)):
        assert L.kman_groups_plan(n, k, 0, mode, byref(wb)) == N.KMAN_EINVAL == R.plan(n, k, False, mode).verdict
        assert wb.value == 0


def test_plan_of_the_edge_sizes():
    """The sizes the edge inputs are built at, derived from make_plan: the
    smallest at which each edge exists."""
    p = R.plan(400_000, 21)
    assert (p.B2, p.C0, p.C1, p.n_tiles0, p.seg_tiles, p.tile) == (1, 320, 1728, 49, 1, 8192)
    p = R.plan(400_000, 21, rc=True)
    assert (p.B2, p.C0, p.C1, p.n_tiles0, p.seg_tiles, p.tile, p.W) == (1, 384, 2880, 98, 2, 4096, 800_000)
    p = R.plan(1_500_000, 21)
    assert (p.B2, p.C0, p.C1, p.n_tiles0, p.seg_tiles) == (1, 448, 4928, 184, 3)
    # chain 1 of a bucket reads anything only past one pass tile of 8192
    # items, which chain 0 spreads over the bucket's 2^B2 sub-regions: a
    # C1h edge on chain 1 needs 2 * C1 >= 8192, which 400 000 bases do not give
    assert 2 * R.plan(400_000, 21).C1 < R.PASS_TILE <= 2 * p.C1
    # C1 = FCAP: rounded up to it from W >> 9 = 5420, clamped from 5462 on
    assert R.plan((5420 << 9) - 1, 21).C1 < R.FCAP == R.plan(5420 << 9, 21).C1 == R.plan(2_800_000, 21).C1
    assert 2_800_000 >> 9 >= 5462
    assert R.plan(2_800_000, 21).B2 == 1 and R.plan(2_800_000, 21).C0 == 512


# every input the GPU tests use: (edge, k, rc, canonical)
# (k = 20: the count items that leave pass 1 as 4 bytes, rest = 31 <= 32 bits)
VARIANTS = [(e, 21, False, False) for e in R.EDGES] + [(e, 20, False, False) for e in R.EDGES] + [
    (R.LATE, 21, False, False),
    ("c0_tile", 9, False, False), ("fin_both", 9, False, False), ("fin_both", 13, False, False),
    ("c0_tile", 21, True, False), ("c1_chain0", 21, True, False), ("fin_both", 21, False, True)]


@pytest.mark.parametrize("edge,k,rc,canonical", VARIANTS)
@pytest.mark.parametrize("delta", [-1, 0, 1])
def test_built_input_hits_its_fills(edge, k, rc, canonical, delta):
    import np_oracle

    c = R.build(edge, delta, k, rc, canonical)
    pl = c.plan
    assert c.fill == c.cap + delta
    recs = np_oracle.parse_fasta(c.text)
    assert len(recs) == 1 and len(recs[0][1]) == R.EDGE_BASES[edge] and set(recs[0][1]) <= set(b"ACGT")
    keys, pos = np_oracle.stream_kmers(recs, k, rc=rc, canonical=canonical)
    f = R.fills(keys, pos, pl)
    for a, b in zip((f.r0, f.sub_lo, f.sub_hi, f.fin), (c.fills.r0, c.fills.sub_lo, c.fills.sub_hi, c.fills.fin)):
        np.testing.assert_array_equal(a, b)
    # fills() is self-consistent
    n = len(keys)
    assert n == (R.EDGE_BASES[edge] - k + 1) * (2 if rc and not canonical else 1)
    assert f.r0.sum() == n and f.fin.sum() == n
    np.testing.assert_array_equal(f.sub_lo[:, 0] + f.sub_hi[:, 1], f.fin)
    np.testing.assert_array_equal(f.sub_hi[:, 0] + f.sub_lo[:, 1], f.fin)
    assert (f.sub_lo <= f.sub_hi).all()
    # the targets, exactly; the edge's own capacity is among them
    found, others = R.capacity_report(c)
    caps = {"r0": pl.C0, "sub": pl.C1, "fin": R.FCAP}
    at_edge = 0
    for (kind, idx, want), got in zip(c.targets, found):
        assert got == ((want, want) if kind == "sub" else want), (kind, idx)
        at_edge += caps[kind] == c.cap and want == c.fill
        if not (caps[kind] == c.cap and want == c.fill):
            assert want <= caps[kind]  # a target beside the edge: inside, by any amount
            assert want < caps[kind] or edge == "fin_m0"  # (there m0 = C1 = FCAP is the point)
    assert at_edge >= 1
    # everything else strictly inside
    for most, cap in others:
        assert 0 <= most < cap
    # the target region holds a repeated key and distinct keys: its own
    # items, pass-0 region (0, s) at the C0 edges, finish region 0 otherwise
    if c.targets[0][0] == "r0":
        seg = (pos >> np.uint64(1)) // np.uint64(pl.tile) % np.uint64(R.RS)
        mine = keys[((keys >> np.uint64(pl.K - R.G1)) == 0) & (seg == c.targets[0][1][1])]
        assert len(mine) == c.fill and sum(c.tile_fills) == c.fill
    else:
        mine = keys[(keys >> np.uint64(pl.rest)) == 0]
        assert len(mine) == c.fills.fin[0]
    u, cnt = np.unique(mine, return_counts=True)
    assert cnt.max() >= 2 and (cnt == 1).sum() >= 2
    if (k, rc, canonical) == (20, False, False):
        assert pl.rest <= 32 < R.plan(R.EDGE_BASES[edge], 21).rest
    if rc:
        assert R.rc_fills(c) == R.RC_FILLS[edge, delta]
    if edge == R.LATE:  # the first two tiles bring the capacity, the third only the item over
        assert c.tile_fills[2] == max(delta, 0) and sum(c.tile_fills[:2]) == c.cap + min(delta, 0)
        assert min(c.tile_fills[:2]) > 0


def test_rc_filler_loads_bucket_255():
    """With -r every item of the A run is also a T...T item: the last bucket's
    regions carry it, and stay inside."""
    for edge in ("c0_tile", "c1_chain0"):
        c, plain = R.build(edge, 0, 21, True), R.build(edge, 0, 21, False)
        assert c.fills.fin[-1] > 2 * plain.fills.fin[-1] + 100  # (twice the items with -r, and the filler's)
        assert c.fills.r0[255].max() < c.plan.C0 and c.fills.sub_hi[-2:].max() < c.plan.C1


def test_fills_bounds_without_alignment():
    """A bucket cut inside a segment: fills() gives the bounds, and they
    differ; a bucket of one pass tile is exact."""
    import np_oracle

    rng = np.random.default_rng(5)
    text = b">r\n" + np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, 2_800_000)].tobytes() + b"\n"
    keys, pos = np_oracle.stream_kmers(np_oracle.parse_fasta(text), 21)
    f = R.fills(keys, pos, R.plan(2_800_000, 21))
    assert (f.sub_lo < f.sub_hi).any() and (f.sub_hi[:, 1] > 0).all()
    c = R.build("c0_tile", 0)
    np.testing.assert_array_equal(c.fills.sub_lo, c.fills.sub_hi)
    assert (c.fills.sub_hi[:, 1] == 0).all()
