"""The k <= 32 window kernels with every event on a tile, thread or pad edge
(tests/extract_cases.py; its premises are asserted in
test_extract_cases_cpu.py): kman_extract (+ d_hist), kman_count_kmers,
kman_kmer_prefix_hist, kman_extract_range, kman_extract_marked and
kman_extract_sorted, called through ctypes on buffers filled with a sentinel.
Every expected value is np_oracle.stream_kmers on the case's records; nothing
may be written past the rows a call reports."""

from __future__ import annotations

from ctypes import byref, c_int, c_uint32, c_uint64, c_void_p

import numpy as np
import pytest

import extract_cases as xc

pytestmark = pytest.mark.gpu

from kman_amd import _native as N  # noqa: E402

SENT8, SENT32, SENT64 = 0xA5, 0xA5A5A5A5, 0xA5A5A5A5A5A5A5A5
GUARD = 64  # sentinel rows after `cap`
FULL = (0, 2 ** 64 - 1)
FLAGS = {"fwd": 0, "rc": N.KMAN_RC, "canon": N.KMAN_CANONICAL, "mixed": N.KMAN_CANONICAL | N.KMAN_MIXED}


class Arena:
    """Device buffers by name, kept across calls and grown when too small."""

    def __init__(self, dev):
        self.dev, self.bufs, self.loaded = dev, {}, None

    def get(self, name, nbytes):
        b = self.bufs.get(name)
        if b is None or b.nbytes < nbytes:
            if b is not None:
                b.free()
            b = self.bufs[name] = self.dev.alloc(max(1 << 20, nbytes + nbytes // 4))
            if name == "codes":
                self.loaded = None
        return b

    def filled(self, name, nbytes, value=SENT8):
        b = self.get(name, nbytes)
        self.dev.memset(b, value, nbytes)
        return b

    def codes(self, case):
        """The case's codes + 64 pad codes in a 16-byte aligned allocation of
        n_bases + 64 rounded up to 16; what follows in the arena reads as 'A'."""
        nb = (case.n_bases + 64 + 15) // 16 * 16
        b = self.get("codes", nb + 256)
        if self.loaded != case.name:
            self.dev.upload(b, np.concatenate([case.codes, np.zeros(nb + 256 - len(case.codes), np.uint8)]))
            self.loaded = case.name
        assert b.ptr % 16 == 0
        return b

    def free(self):
        for b in self.bufs.values():
            b.free()
        self.bufs = {}


@pytest.fixture(scope="module")
def A():
    from kman_amd import engine

    a = Arena(engine.default_device())
    yield a
    a.free()


def _bound(case, variant):
    return case.n_bases * (2 if variant == "rc" else 1)


def _extract(A, case, k, variant, pos_bytes, cap, key_range=FULL, hist_lo=None):
    """One kman_extract (kman_extract_range for a key range) -> (rc, n_kmers,
    all cap + 64 key rows, all pos rows or None, the 8 x 256 table or None)."""
    dev, rows = A.dev, cap + GUARD
    d_codes = A.codes(case)
    d_keys = A.filled("keys", 8 * rows)
    d_pos = A.filled("pos", pos_bytes * rows) if pos_bytes else None
    flags = FLAGS[variant] | (N.KMAN_WANT_POS if pos_bytes else 0)
    d_hist = None
    if hist_lo is not None:
        d_hist = A.filled("hist", 8 * 256 * 8, 0)
        flags |= N.KMAN_HIST_LO(hist_lo)
    n = c_uint64(0)
    tail = (c_void_p(d_keys.ptr), c_void_p(d_pos.ptr if d_pos else None), pos_bytes, cap,
            c_void_p(d_hist.ptr if d_hist else None), byref(n))
    if key_range == FULL:
        rc = N.lib().kman_extract(dev.ctx, c_void_p(d_codes.ptr), case.n_bases, k, flags, *tail)
    else:
        rc = N.lib().kman_extract_range(dev.ctx, c_void_p(d_codes.ptr), case.n_bases, k, flags, key_range[0],
                                        key_range[1], *tail)
    dev.sync()
    keys = dev.download(d_keys, rows, np.uint64)
    pos = dev.download(d_pos, rows, np.uint32 if pos_bytes == 4 else np.uint64) if pos_bytes else None
    hist = dev.download(d_hist, 8 * 256, np.uint64).reshape(8, 256) if d_hist else None
    return rc, int(n.value), keys, pos, hist


def _sent(a):
    return SENT32 if a.dtype == np.uint32 else SENT64


def _check_rows(got, want_keys, want_pos, msg, written=None):
    """rc OK, the count, rows [0, n) equal to the stream, every later row
    sentinel (written: only that many rows were written, the rest counted)."""
    rc, n, keys, pos, _ = got
    assert n == len(want_keys), "%s: n_kmers %d, expected %d" % (msg, n, len(want_keys))
    w = n if written is None else written
    np.testing.assert_array_equal(keys[:w], want_keys[:w], err_msg=msg + " keys")
    assert np.all(keys[w:] == SENT64), msg + ": keys written past row %d" % w
    if pos is not None:
        np.testing.assert_array_equal(pos[:w], want_pos[:w].astype(pos.dtype), err_msg=msg + " pos")
        assert np.all(pos[w:] == _sent(pos)), msg + ": pos written past row %d" % w


def _check_untouched(got, msg):
    assert np.all(got[2] == SENT64), msg + ": keys written"
    assert got[3] is None or np.all(got[3] == _sent(got[3])), msg + ": pos written"


def _count(A, case, k, variant):
    n = c_uint64(SENT64)
    rc = N.lib().kman_count_kmers(A.dev.ctx, c_void_p(A.codes(case).ptr), case.n_bases, k, FLAGS[variant], byref(n))
    assert rc == N.KMAN_OK, case.name
    return int(n.value)


# --------------------------------------------------------------- kman_extract

FAMILY = {"A": xc.family_a, "B": xc.family_b, "C": xc.family_c, "D": xc.family_d, "E": xc.family_e, "F": xc.family_f}


@pytest.mark.parametrize("variant", xc.VARIANTS)
@pytest.mark.parametrize("family", "ABCDEF")
def test_extract_family(A, family, variant):
    """Every case: u64 pos at the trivial bound, u32 pos at the exact count
    (sized by kman_count_kmers), no pos, and one row short of the count."""
    for case in FAMILY[family]():
        k, msg = case.k, "%s %s" % (case.name, variant)
        wk, wp = case.expected(variant)
        bound = _bound(case, variant)
        got = _extract(A, case, k, variant, 8, bound)
        assert got[0] == N.KMAN_OK, msg
        _check_rows(got, wk, wp, msg + " cap=bound")
        got = _extract(A, case, k, variant, 4, len(wk))
        assert got[0] == N.KMAN_OK, msg
        _check_rows(got, wk, wp, msg + " cap=count")
        got = _extract(A, case, k, variant, 0, bound)
        assert got[0] == N.KMAN_OK, msg
        _check_rows(got, wk, wp, msg + " no pos")
        if len(wk):
            got = _extract(A, case, k, variant, 8, len(wk) - 1)
            assert got[0] == N.KMAN_ECAP, msg
            _check_untouched(got, msg + " cap=count-1")


def _hist_cases():
    for k in xc.K:
        yield next(c for c in xc.family_a((k,)) if c.n_bases == 4096 + k - 1)
        yield xc.event_case("B", k, 4096, -1, "n")
        yield next(xc.family_d((k,), (4096,)))
    yield from (c for c in xc.family_c((5, 32), (2048,)) if c.meta["d"] == 0)
    yield from (c for c in xc.family_e() if c.meta["tile"] == 4096 and "sparse" in c.name)
    yield from (c for c in xc.family_f() if c.meta["kind"] == "poly_acgt")


def _plan(lo, hi):
    np_, sh, bi = c_uint32(0), (c_uint32 * 8)(), (c_uint32 * 8)()
    assert N.lib().kman_sort_plan_range(lo, hi, byref(np_), sh, bi) == N.KMAN_OK
    return [(int(sh[p]), int(bi[p])) for p in range(np_.value)]


@pytest.mark.parametrize("variant", xc.VARIANTS)
def test_extract_hist(A, variant):
    """d_hist with KMAN_HIST_LO(lo): every pass of kman_sort_plan_range(lo, 2k)
    is the bincount of the stream's digits, the other rows stay zero.  lo == 2k
    is the empty plan of the header's "bits [b, 2k)": KMAN_OK, the keys
    written, the table untouched."""
    for case in _hist_cases():
        k = case.k
        wk, wp = case.expected(variant)
        for lo in sorted({0, max(2 * k - 8, 0), 2 * k - 1, 2 * k}):
            msg = "%s %s lo=%d" % (case.name, variant, lo)
            got = _extract(A, case, k, variant, 0, _bound(case, variant), hist_lo=lo)
            assert got[0] == N.KMAN_OK, msg
            _check_rows(got, wk, wp, msg)
            plan = _plan(lo, 2 * k)
            assert len(plan) == (2 * k - lo + 7) // 8
            want = np.zeros((8, 256), np.uint64)
            for p, (sh, bi) in enumerate(plan):
                d = (wk >> np.uint64(sh)) & np.uint64((1 << bi) - 1)
                want[p] = np.bincount(d.astype(np.int64), minlength=256)
            np.testing.assert_array_equal(got[4], want, err_msg=msg)


# ----------------------------------------------------------- kman_count_kmers


@pytest.mark.parametrize("variant", xc.VARIANTS)
def test_count_kmers(A, variant):
    """The oracle's count on every case: doubled for -r, not for canonical."""
    for case in xc.small_cases():
        k = case.k or 13
        nf = len(case.expected("fwd", k)[0])
        assert _count(A, case, k, variant) == nf * (2 if variant == "rc" else 1), "%s %s" % (case.name, variant)


# ------------------------------------------------------ kman_kmer_prefix_hist


def _prefix_hist(A, case, k, variant):
    d_hist = A.filled("hist", 8 * 256 * 8)
    n = c_uint64(SENT64)
    rc = N.lib().kman_kmer_prefix_hist(A.dev.ctx, c_void_p(A.codes(case).ptr), case.n_bases, k, FLAGS[variant],
                                       c_void_p(d_hist.ptr), byref(n))
    A.dev.sync()
    assert rc == N.KMAN_OK, case.name
    h = A.dev.download(d_hist, 8 * 256, np.uint64)
    assert np.all(h[256:] == SENT64), case.name + ": written past 256 bins"
    return int(n.value), h[:256]


def _check_prefix_hist(A, case, k, variant):
    wk = case.expected(variant, k)[0]
    top = min(8, 2 * k)
    want = np.bincount((wk >> np.uint64(2 * k - top)).astype(np.int64), minlength=256)
    n, h = _prefix_hist(A, case, k, variant)
    assert n == len(wk), "%s %s" % (case.name, variant)
    np.testing.assert_array_equal(h, want.astype(np.uint64), err_msg="%s %s" % (case.name, variant))


@pytest.mark.parametrize("variant", ["fwd", "rc"])
@pytest.mark.parametrize("family", "ABE")
def test_prefix_hist(A, family, variant):
    cases = {"A": xc.family_a, "B": lambda: xc.family_b(xc.K), "E": lambda: xc.family_e(xc.K)}[family]()
    for case in cases:
        _check_prefix_hist(A, case, case.k, variant)


# ------------------------------------------------------------- the large case


def _second_tile_premise():
    """4099 tiles > 8 blocks of 256 threads on every CU: some persistent block
    takes a second tile."""
    import ctypes

    from kman_amd import engine

    hip = ctypes.CDLL("libamdhip64.so")  # (the runtime the library itself is linked to)
    cus = c_int(0)
    # 63: hipDeviceAttributeMultiprocessorCount (hip_runtime_api.h, hipDeviceAttribute_t)
    assert hip.hipDeviceGetAttribute(byref(cus), 63, engine.default_device().index) == 0
    assert 0 < cus.value and xc.H_TILES > 8 * cus.value, "%d CUs" % cus.value


def test_large_count_kmers(A):
    """count_kernel's grid stride: 4099 tiles against 4096 blocks."""
    h = xc.family_h()
    assert xc.H_TILES > xc.COUNT_GRID
    nf = len(h.expected("fwd")[0])
    for variant in xc.VARIANTS:
        assert _count(A, h, h.k, variant) == nf * (2 if variant == "rc" else 1), variant


def test_large_prefix_hist(A):
    """kmer_hist_kernel's second tile and the codes prefetched for it."""
    _second_tile_premise()
    h = xc.family_h()
    for variant in ("fwd", "rc"):
        _check_prefix_hist(A, h, h.k, variant)


def test_large_extract(A):
    """extract_kernel's persistent loop, sized by the count (u32 pos)."""
    _second_tile_premise()
    h = xc.family_h()
    for variant in ("fwd", "rc"):
        wk, wp = h.expected(variant)
        got = _extract(A, h, h.k, variant, 4, len(wk))
        assert got[0] == N.KMAN_OK
        _check_rows(got, wk, wp, "%s %s" % (h.name, variant))


# --------------------------------------------------------- kman_extract_range


def _ranges(ks, mask):
    x0, xm, x1 = int(ks[0]), int(ks[len(ks) // 2]), int(ks[-1])
    out = [FULL, (x0, x0), (xm, xm), (x1, x1), (0, 0), (mask, mask), (xm + 1, xm) if xm < mask else (1, 0)]
    gaps = np.nonzero(np.diff(ks) > np.uint64(1))[0]
    for i in gaps[[0, len(gaps) // 2, -1]] if len(gaps) else []:
        out.append((int(ks[i]) + 1, int(ks[i + 1]) - 1))
    return out


@pytest.mark.parametrize("variant", ["fwd", "rc", "canon"])
@pytest.mark.parametrize("k", xc.K_SUB)
def test_extract_range(A, k, variant):
    mask = (1 << (2 * k)) - 1
    cases = [xc.event_case("B", k, 4096, -1, "n"),
             next(c for c in xc.family_e((k,)) if c.name.endswith("sparse_t4096")),
             next(c for c in xc.family_f((k,)) if c.meta["kind"] == "poly_acgt")]
    pos_bytes = 4 if variant == "canon" else 8
    for case in cases:
        wk, wp = case.expected(variant)
        ks = np.unique(wk)
        cap = _bound(case, variant)
        for lo, hi in _ranges(ks, mask):
            msg = "%s %s [%x, %x]" % (case.name, variant, lo, hi)
            sel = (wk >= np.uint64(lo)) & (wk <= np.uint64(hi)) if lo <= hi else np.zeros(len(wk), bool)
            got = _extract(A, case, k, variant, pos_bytes, cap, (lo, hi))
            assert got[0] == N.KMAN_OK, msg
            _check_rows(got, wk[sel], wp[sel], msg)
        # one row short of a range holding m >= 2 keys: counted, not written
        lo, hi = int(ks[len(ks) // 4]), int(ks[3 * len(ks) // 4])
        assert (lo, hi) != FULL
        sel = (wk >= np.uint64(lo)) & (wk <= np.uint64(hi))
        m = int(np.count_nonzero(sel))
        assert m >= 2
        got = _extract(A, case, k, variant, pos_bytes, m - 1, (lo, hi))
        assert got[0] == N.KMAN_ECAP, case.name
        _check_rows(got, wk[sel], wp[sel], "%s %s cap=m-1" % (case.name, variant), written=m - 1)
        got = _extract(A, case, k, variant, pos_bytes, m, (lo, hi))
        assert got[0] == N.KMAN_OK, case.name
        _check_rows(got, wk[sel], wp[sel], "%s %s cap=m" % (case.name, variant))


# -------------------------------------------------------- kman_extract_marked

MARKED = [(2, 1), (2, 4), (5, 10), (8, 16), (9, 16), (9, 17), (21, 16), (21, 17), (21, 20)]


@pytest.mark.parametrize("variant", ["fwd", "rc", "canon"])
@pytest.mark.parametrize("k,map_bits", MARKED)
def test_extract_marked(A, k, map_bits, variant):
    """The coarse bitmap at min(2k, 16) map bits (exact) and above (a
    prefilter).  Tiles place their rows with an atomic: the multiset of
    (key, pos) is the filtered stream's, and one tile's rows are contiguous
    and in stream order."""
    dev, val = A.dev, 2
    T = xc.TILE_EXTRACT_RC if variant == "rc" else xc.TILE_EXTRACT
    rng = np.random.default_rng(100 * k + map_bits)
    maps = {"random": rng.integers(0, 4, 1 << map_bits, dtype=np.uint8),
            "none": np.zeros(1 << map_bits, np.uint8), "all": np.full(1 << map_bits, val, np.uint8)}
    cases = [xc.event_case("B", k, 4096, 0, "start"),
             next(c for c in xc.family_e((k,)) if c.name.endswith("sparse_t4096"))]
    for case in cases:
        wk, wp = case.expected(variant)
        cap = _bound(case, variant)
        for mname, pm in maps.items():
            msg = "%s %s map=%s" % (case.name, variant, mname)
            sel = pm[(wk >> np.uint64(2 * k - map_bits)).astype(np.int64)] == val
            d_map = A.get("map", len(pm))
            dev.upload(d_map, pm)
            d_keys, d_pos = A.filled("keys", 8 * (cap + GUARD)), A.filled("pos", 8 * (cap + GUARD))
            n = c_uint64(SENT64)
            rc = N.lib().kman_extract_marked(dev.ctx, c_void_p(A.codes(case).ptr), case.n_bases, k,
                                             FLAGS[variant] | N.KMAN_WANT_POS, c_void_p(d_map.ptr), map_bits, val,
                                             c_void_p(d_keys.ptr), c_void_p(d_pos.ptr), 8, cap, byref(n))
            dev.sync()
            assert rc == N.KMAN_OK and n.value == np.count_nonzero(sel), msg
            keys, pos = dev.download(d_keys, cap + GUARD, np.uint64), dev.download(d_pos, cap + GUARD, np.uint64)
            m = int(n.value)
            assert np.all(keys[m:] == SENT64) and np.all(pos[m:] == SENT64), msg
            if mname == "none":
                assert m == 0
            if mname == "all":
                assert m == len(wk)
            o = np.argsort(pos[:m], kind="stable")  # (pos is unique: window << 1 | strand)
            np.testing.assert_array_equal(pos[:m][o], wp[sel], err_msg=msg)
            np.testing.assert_array_equal(keys[:m][o], wk[sel], err_msg=msg)
            tile = (pos[:m] >> np.uint64(1)).astype(np.int64) // T
            runs = tile[np.concatenate([[True], tile[1:] != tile[:-1]])] if m else tile
            assert len(runs) == len(np.unique(tile)), msg + ": a tile's rows are not contiguous"
            same = tile[1:] == tile[:-1]
            assert np.all(pos[:m][1:][same] > pos[:m][:-1][same]), msg + ": a tile's rows out of stream order"


# -------------------------------------------------------- kman_extract_sorted


def _split_bits(n, key_bits):
    lo = c_uint32(0)
    assert N.lib().kman_split_bits(n, key_bits, byref(lo)) == N.KMAN_OK
    return int(lo.value)


def _sorted(A, case, k, variant, pos_bytes, lo_bit, cap):
    dev, rows = A.dev, cap + GUARD
    d = [A.filled(nm, 8 * rows) for nm in ("keys", "keys_alt")]
    d += [A.filled(nm, pos_bytes * rows) if pos_bytes else None for nm in ("pos", "pos_alt")]
    n, alt = c_uint64(SENT64), c_int(-1)
    ptr = [c_void_p(b.ptr if b else None) for b in d]
    rc = N.lib().kman_extract_sorted(dev.ctx, c_void_p(A.codes(case).ptr), case.n_bases, k,
                                     FLAGS[variant] | (N.KMAN_WANT_POS if pos_bytes else 0), lo_bit, ptr[0], ptr[1],
                                     ptr[2], ptr[3], pos_bytes, cap, byref(n), byref(alt))
    dev.sync()
    pt = np.uint32 if pos_bytes == 4 else np.uint64
    out = [dev.download(d[0], rows, np.uint64), dev.download(d[1], rows, np.uint64)]
    out += [dev.download(b, rows, pt) if b else None for b in d[2:]]
    return rc, int(n.value), alt.value, out


def _check_sorted(A, case, k, variant, pos_bytes, lo_bit, stream, msg, cap=None):
    wk, wp = stream
    pre = wk >> np.uint64(lo_bit) if lo_bit < 64 else np.zeros(len(wk), np.uint64)
    o = np.argsort(pre, kind="stable")
    cap = len(wk) if cap is None else cap
    rc, n, alt, (k0, k1, p0, p1) = _sorted(A, case, k, variant, pos_bytes, lo_bit, cap)
    assert rc == N.KMAN_OK and n == len(wk) and alt in (0, 1), msg
    keys, other = (k1, k0) if alt else (k0, k1)
    np.testing.assert_array_equal(keys[:n], wk[o], err_msg=msg + " keys")
    assert np.all(keys[n:] == SENT64) and np.all(other[n:] == SENT64), msg + ": keys written past row n"
    if pos_bytes:
        pos, other = (p1, p0) if alt else (p0, p1)
        np.testing.assert_array_equal(pos[:n], wp[o].astype(pos.dtype), err_msg=msg + " pos")
        assert np.all(pos[n:] == _sent(pos)) and np.all(other[n:] == _sent(pos)), msg + ": pos written past row n"


def _lo_bits(n, k):
    return sorted({0, _split_bits(n, 2 * k), max(2 * k - 7, 0), 2 * k - 1})


@pytest.mark.parametrize("variant", ["fwd", "rc"])
@pytest.mark.parametrize("k", [2, 13, 21, 25])
def test_extract_sorted_segments(A, k, variant):
    """Family G: fewer window tiles than the 8 segments, as many, and more
    (the fused extract_pass; cap == n)."""
    cases = [c for c in xc.family_g() if c.meta["rc"] == (variant == "rc")]
    assert [c.meta["tiles"] for c in cases] == list(xc.G_COUNTS)
    for case in cases:
        stream = case.expected(variant, k)
        for lo_bit in _lo_bits(len(stream[0]), k):
            for pos_bytes in (4, 0):
                _check_sorted(A, case, k, variant, pos_bytes, lo_bit, stream,
                              "%s k=%d %s lo=%d pos=%d" % (case.name, k, variant, lo_bit, pos_bytes))


@pytest.mark.parametrize("variant", ["fwd", "rc"])
@pytest.mark.parametrize("k", [2, 13, 21, 25])
def test_extract_sorted_events(A, k, variant):
    """Family B's events at the edge of extract_pass's forward tile."""
    for case in xc.family_b((k,), (8192,), both=False):
        stream = case.expected(variant)
        for lo_bit in _lo_bits(len(stream[0]), k):
            for pos_bytes in (4, 0):
                _check_sorted(A, case, k, variant, pos_bytes, lo_bit, stream,
                              "%s %s lo=%d pos=%d" % (case.name, variant, lo_bit, pos_bytes))


def test_extract_sorted_other_routes(A):
    """The routes that run kman_extract + kman_sort_range: k > 25, canonical
    keys, u64 pos, lo_bit == 2k (nothing to sort by: stream order)."""
    g = next(c for c in xc.family_g() if c.meta["tiles"] == 9 and not c.meta["rc"])
    for k, variant, pos_bytes, lo_bit in ((26, "fwd", 4, 20), (21, "canon", 4, 21), (21, "rc", 8, 21), (21, "fwd", 4, 42),
                                          (32, "fwd", 4, 64)):
        stream = g.expected(variant, k)
        _check_sorted(A, g, k, variant, pos_bytes, lo_bit, stream, "%s k=%d %s lo=%d" % (g.name, k, variant, lo_bit),
                      cap=_bound(g, variant))


@pytest.mark.parametrize("variant", ["fwd", "rc"])
def test_extract_sorted_capacity(A, variant):
    """cap == n passes (every fused test above); cap == n - 1 is KMAN_ECAP with
    nothing written; an input without a k-mer is KMAN_OK with nothing written."""
    k = 21
    for case in [c for c in xc.family_g() if c.meta["tiles"] in (2, 9)] + [xc.event_case("B", k, 8192, 0, "n")]:
        n = len(case.expected(variant, k)[0])
        rc, got, alt, bufs = _sorted(A, case, k, variant, 4, 21, n - 1)
        assert rc == N.KMAN_ECAP, case.name
        for b in bufs:
            assert np.all(b == _sent(b)), case.name + ": written on KMAN_ECAP"
    for case in [c for c in xc.family_e() if c.name.endswith("all_n")]:
        for pos_bytes in (4, 0):
            rc, n, alt, bufs = _sorted(A, case, case.k, variant, pos_bytes, 0, 16)
            assert (rc, n, alt) == (N.KMAN_OK, 0, 0), case.name
            for b in bufs:
                assert b is None or np.all(b == _sent(b)), case.name + ": written without a k-mer"


# ------------------------------------------------------------ one engine pass


def test_engine_codes_and_keys(A):
    """The parser's codes for the FASTA of a case are the hand-built ones, and
    engine.extract gives the same stream."""
    from kman_amd import engine

    dev = A.dev
    for case in (xc.event_case("B", 21, 4096, -1, "n"), xc.event_case("B", 32, 8192, 0, "start"),
                 xc.event_case("B", 2, 2048, -1, "start_then_n")):
        p = engine.parse(dev, xc.fasta_text(case))
        km = None
        try:
            assert (p.n_bases, p.n_records) == (case.n_bases, len(case.records))
            np.testing.assert_array_equal(dev.download(p.codes, p.n_bases + 64, np.uint8), case.codes, err_msg=case.name)
            wk, wp = case.expected("fwd")
            km = engine.extract(p, case.k, False, True)
            assert km.n == len(wk) and km.pos_bytes == 4
            np.testing.assert_array_equal(dev.download(km.keys, km.n, np.uint64), wk, err_msg=case.name)
            np.testing.assert_array_equal(dev.download(km.pos, km.n, np.uint32), wp.astype(np.uint32), err_msg=case.name)
        finally:
            if km is not None:
                km.free()
            p.free()
