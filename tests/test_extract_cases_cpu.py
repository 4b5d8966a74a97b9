"""The premises of test_gpu_extract_edges.py, checked without a GPU: the two
statements of the expected stream agree on every case of tests/extract_cases.py,
and every family holds the edges it promises."""

from __future__ import annotations

import numpy as np
import pytest

import extract_cases as xc


@pytest.fixture(scope="module")
def cases():
    return list(xc.small_cases())


def _agree(case, k, msg):
    w = xc.code_windows(case.codes, case.n_bases, k)
    for v in xc.VARIANTS:
        k1, p1 = case.expected(v, k)
        k2, p2 = xc.code_stream(case.codes, case.n_bases, k, v, w)
        np.testing.assert_array_equal(k1, k2, err_msg="%s %s keys" % (msg, v))
        np.testing.assert_array_equal(p1, p2, err_msg="%s %s pos" % (msg, v))


def test_case_names_are_unique_and_every_family_is_there(cases):
    assert len({c.name for c in cases}) == len(cases)
    assert {c.family for c in cases} == set("ABCDEFG")
    for c in cases:
        assert c.codes.dtype == np.uint8 and len(c.codes) == c.n_bases + 64 and np.all(c.codes[c.n_bases:] == 4)
        assert c.n_bases <= 20_500 + 2 * 4096 or c.family in "EG", c.name


@pytest.mark.parametrize("family", "ABCDEF")
def test_the_two_statements_agree(cases, family):
    some = [c for c in cases if c.family == family]
    assert some
    for c in some:
        _agree(c, c.k, c.name)


def test_the_two_statements_agree_on_family_g(cases):
    for c in (c for c in cases if c.family == "G"):
        for k in (2, 13, 25):
            _agree(c, k, "%s k=%d" % (c.name, k))


def test_the_plain_window_loop_agrees():
    """code_windows against the same rule in Python integers, on cases short
    enough for it: lengths around k, and events of every kind cut to 3k codes."""
    small = [c for c in xc.family_a() if c.n_bases <= 40]
    for k in xc.K:
        for kind in ("n", "start", "nstart", "n_then_start", "start_then_n"):
            c = xc.event_case("B", k, 2048, -1, kind)
            lo = c.meta["p"] - k - 3
            small.append(_cut(c, lo, 3 * k + 8))
    assert len(small) > 60
    for c in small:
        s, f, r = xc.code_windows(c.codes, c.n_bases, c.k)
        got = [(int(a), int(b), int(d)) for a, b, d in zip(s, f, r)]
        assert got == xc.code_stream_plain(c.codes, c.n_bases, c.k), c.name


class _cut:
    """Codes [lo, lo + n) of a case, as a case of their own."""

    def __init__(self, c, lo, n):
        self.name, self.k, self.n_bases = c.name + "_cut", c.k, n
        self.codes = np.concatenate([c.codes[lo:lo + n], np.full(64, 4, np.uint8)])


def test_raw_codes_are_raw(cases):
    raw = [c for c in cases if c.family == "C"]
    seen = {int(c.codes[c.meta["p"]]) for c in raw}
    assert seen == set(xc.RAW_N) | set(xc.RAW_START)
    for c in raw:
        twin = xc.np_oracle.codes_of(c.records)[0]
        diff = np.nonzero(twin != c.codes[:c.n_bases])[0]
        # (12 itself is among the raw record starts: that case is its own twin)
        assert list(diff) == ([] if c.meta["raw"] == 12 else [c.meta["p"]]) and twin[c.meta["p"]] in (4, 12), c.name
    assert {(c.k, c.meta["e"], c.meta["d"], c.meta["kind"]) for c in raw} == {
        (k, e, d, kind) for k in (5, 32) for e in xc.E for d in xc.deltas(k) for kind in ("n", "nstart")}


def test_family_b_covers_the_grid(cases):
    b = [c for c in cases if c.family == "B"]
    have = {(c.meta["e"], c.meta["d"], c.k, c.meta["kind"]) for c in b}
    for k in xc.K + (21,):
        want_d = {-k, -k + 1, -16, -8, -1, 0, 1, 7, 8, 15, 16, k - 2, k - 1}
        assert set(xc.deltas(k)) == want_d
        for e in xc.E:
            for d in want_d:
                assert (e, d, k, "n") in have and (e, d, k, "start") in have, (e, d, k)
    for k in xc.K_SUB:
        for e in xc.E:
            assert (e, -1, k, "n_then_start") in have and (e, -1, k, "start_then_n") in have
    for c in b:  # the record reaches two tiles past e
        assert c.n_bases >= c.meta["e"] + 2 * 4096


def test_family_b_and_c_lose_exactly_the_predicted_windows(cases):
    bases = {}
    for c in (c for c in cases if c.family in "BC"):
        at = (c.meta["e"], c.k)
        if at not in bases:
            bases[at] = xc.record_stream([(b"r", xc.base_record(at[0]))], c.k, "fwd")
        base = bases[at]
        kk, pp = xc.code_stream(c.codes, c.n_bases, c.k, "fwd")
        s0 = (base[1] >> np.uint64(1)).astype(np.int64)
        s1 = (pp >> np.uint64(1)).astype(np.int64)
        lost = set(s0.tolist()) - set(s1.tolist())
        assert lost == xc.gone(c) and lost, c.name
        assert set(s1.tolist()) <= set(s0.tolist())
        np.testing.assert_array_equal(kk, base[0][np.isin(s0, s1)], err_msg=c.name)  # the rest keep their keys
    # the two promised rules, spelled out once
    c = xc.event_case("B", 21, 4096, 0, "start")
    assert xc.gone(c) == set(range(4096 - 20, 4096))
    c = xc.event_case("B", 21, 4096, 0, "n")
    assert xc.gone(c) == set(range(4096 - 20, 4097))


def test_family_d_runs_cross_the_edge(cases):
    d = [c for c in cases if c.family == "D"]
    assert {(c.k, c.meta["e"]) for c in d} == {(k, e) for k in xc.K for e in (2048, 4096, 8192)}
    for c in d:
        a, z = c.meta["run"]
        k, e = c.k, c.meta["e"]
        assert a == e - 3 * k and e + 3 * k <= z < e + 4 * k
        starts = np.nonzero(c.codes[:c.n_bases] & 8)[0]
        lens = np.diff(starts[(starts >= a) & (starts <= z)])
        assert set(lens.tolist()) <= {k, k - 1, 1} and len(lens) >= 6
        assert np.any((starts > e - k) & (starts <= e)) or k == 2


def test_family_e_tiles_hold_the_promised_windows(cases):
    e = [c for c in cases if c.family == "E"]
    assert {c.k for c in e} == set(xc.K_SUB)
    seen_tiles = set()
    for c in e:
        T = c.meta["tile"]
        _, pos = c.expected("fwd")
        got = xc.tile_counts(pos, c.n_bases, T)
        assert got.tolist() == c.meta["counts"], c.name
        starts = (pos >> np.uint64(1)).astype(np.int64)
        for t, s in c.meta.get("single", {}).items():
            assert starts[starts // T == t].tolist() == [s] and s in (t * T, (t + 1) * T - 1), c.name
        if "wave" in c.meta:
            W = c.meta["wave"]
            assert all(a != b for a, b in zip(c.meta["waves"], c.meta["waves"][1:]))
            for t, w in enumerate(c.meta["waves"]):
                np.testing.assert_array_equal(starts[starts // T == t], t * T + w * W + np.arange(W))
        if "sparse" in c.name:
            seen_tiles.add(T)
        if "all_n" in c.name:
            assert len(pos) == 0
            for T2 in (2048, 4096):
                assert not xc.tile_counts(pos, c.n_bases, T2).any()
    assert seen_tiles == {2048, 4096, 8192}
    assert {(c.meta["tile"], c.meta["wave"]) for c in e if "wave" in c.meta} == set(xc.E_WAVES)


def test_family_a_interval_holds_every_residue(cases):
    n = [c.n_bases for c in cases if c.meta.get("interval")]
    assert n == list(range(4096 - 80, 4096 + 17))
    for side in ([x for x in n if x + 64 < 4096 + 64], [x for x in n if x + 64 > 4096 + 64]):
        assert {x % 16 for x in side} == set(range(16)) and {(x + 64) % 16 for x in side} == set(range(16))
    a = {(c.k, c.n_bases) for c in cases if c.family == "A"}
    for k in xc.K:
        for x in [1, k - 1, k, k + 1] + [e + d for e in xc.E for d in (-1, 0, 1, k - 2, k - 1, k)]:
            assert (k, x) in a


def test_family_f_keys(cases):
    f = {c.name: c for c in cases if c.family == "F"}
    for k in (31, 32):
        mask = (1 << (2 * k)) - 1
        kf = f["f_k%d_poly_a" % k].expected("fwd")[0]
        assert len(kf) > 4096 and not kf.any()
        assert np.all(f["f_k%d_poly_t" % k].expected("fwd")[0] == np.uint64(mask))
        kr = f["f_k%d_poly_acgt" % k].expected("rc")[0]
        assert kr.min() == 0 and kr.max() == np.uint64(mask)
        s, fw, rc = xc.code_windows(f["f_k%d_alternate" % k].codes, 4296, k)
        lt = fw < rc
        assert np.count_nonzero(lt[1:] != lt[:-1]) > 1000 and 1000 < np.count_nonzero(lt) < len(lt) - 1000
    s, fw, rc = xc.code_windows(f["f_k32_palindrome"].codes, f["f_k32_palindrome"].n_bases, 32)
    assert len(s) > 4096 and np.array_equal(fw, rc)


def test_family_g_tile_counts(cases):
    g = [c for c in cases if c.family == "G"]
    for win in (8192, 4096):
        assert [-(-c.n_bases // win) for c in g if c.meta["win"] == win] == [1, 2, 7, 8, 9, 17]
    assert xc.NSEG == 8 and min(xc.G_COUNTS) < 8 < max(xc.G_COUNTS) and 8 in xc.G_COUNTS
    for c in g:
        assert np.all(c.codes[:c.n_bases] & 4 == 0)


def test_family_h_has_more_tiles_than_the_count_grid():
    h = xc.family_h()
    assert h.n_bases == 4099 * 4096 - 5 and -(-h.n_bases // 4096) == 4099 > xc.COUNT_GRID
    assert 200 <= len(h.records) <= 500
    keys, pos = h.expected("fwd")
    assert 1_500_000 < len(keys) < 2_500_000
    counts = xc.tile_counts(pos, h.n_bases, 4096)
    assert counts[4096:].sum() > 0 and np.count_nonzero(counts == 0) > 3000
    cut = 3 * (h.n_bases // 300)  # (the second statement on the first stretches)
    np.testing.assert_array_equal(keys[pos < np.uint64(2 * (cut - h.k + 1))], xc.code_stream(h.codes, cut, h.k, "fwd")[0])
