"""The k > 32 entry points called directly through the C ABI at their tile and
word edges, against the plain-Python statement of wide_cases.py:

  kman_extract_wide / kman_extract_words   events at the 2048-window tile
      edges, all-A / all-T keys, palindromes, ties of the first word, both
      pos widths, count-only calls, KMAN_ECAP, strides, refusals
  kman_rle_wide / kman_rle_words           group layouts at the 4096 / 2048
      row tile edges, every value width, the all-ones key, strides
  kman_iota_u64, kman_gather, kman_or_u64, kman_widen_u32, kman_batch_tags,
  kman_tag_batches, kman_memcpy_d2d        past one grid stride of 8192 x 256
  kman_format_*_wide(_dev), kman_format_*_words(_dev)   host == device ==
      reference text, around the 32 768-byte LDS staging limit (k = 61)
  the k in 33..64 pipeline of INTEGRATION.md, call by call.

Every comparison is exact."""

from __future__ import annotations

from ctypes import byref, c_int, c_size_t, c_uint64, c_void_p

import numpy as np
import pytest

import wide_cases as wc

pytestmark = pytest.mark.gpu

GUARD = 64  # rows of 0x5A kept after every output array
KS = [33, 34, 48, 63, 64]
KS_LONG = [65, 96, 97, 129]


@pytest.fixture(scope="module")
def dev():
    from kman_amd import engine

    return engine.default_device()


def _N():
    from kman_amd import _native as N

    return N


def P(x):
    return None if x is None else c_void_p(x)


class Bufs:
    """Device buffers of one test step, freed together."""

    def __init__(self, dev):
        self.dev, self.all = dev, []

    def alloc(self, nbytes, fill=None):
        nbytes = max(16, int(nbytes))
        b = self.dev.alloc(nbytes)
        self.all.append(b)
        if fill is not None:
            self.dev.memset(b, fill, nbytes)
        return b

    def put(self, a):
        a = np.ascontiguousarray(a)
        b = self.alloc(a.nbytes)
        if a.nbytes:
            self.dev.upload(b, a)
        return b

    def free(self):
        for b in self.all:
            b.free()
        self.all = []

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.free()


def _untouched(a) -> bool:
    return bool((np.ascontiguousarray(a).view(np.uint8) == 0x5A).all())


# ================================================================ extraction
_WORDS = {}


def _to_words(w):
    t = _WORDS.get(w)
    if t is None:
        if len(_WORDS) > 400000:
            _WORDS.clear()
        t = _WORDS[w] = wc.to_words(w)
    return t


def _refs(recs, k):
    """{flags: (rows (n, W) u64, pos (n,) u64)} for no flag, KMAN_RC and
    KMAN_CANONICAL, from one pass over the valid windows."""
    N = _N()
    W = wc.nwords(k)
    valid = wc.valid_starts(recs, k)
    plain, both, canon = [], [], []
    for g, w in valid:
        r = wc.revcomp(w)
        f_, r_ = _to_words(w), _to_words(r)
        plain.append(f_)
        both.append(f_)
        both.append(r_)
        canon.append(f_ if w <= r else r_)
    gp = np.array([g << 1 for g, _ in valid], dtype=np.uint64)
    bp = np.empty(2 * len(valid), np.uint64)
    bp[0::2] = gp
    bp[1::2] = gp | np.uint64(1)

    def arr(x):
        return np.array(x, dtype=np.uint64).reshape(len(x), W)

    return {0: (arr(plain), gp), N.KMAN_RC: (arr(both), bp), N.KMAN_CANONICAL: (arr(canon), gp)}


def _extract(dev, p, k, flags, entry, total, pos_bytes=8, cap=None, pad=0, want_pos=True):
    """One call of kman_extract_wide ("wide") or kman_extract_words ("words")
    into 0x5A-filled buffers of cap rows (+ pad rows between the word planes)
    + GUARD.  -> (rc, n, rows (m, W), pos (m,) or None, guard untouched)."""
    N = _N()
    L = N.lib()
    W = wc.nwords(k)
    cap = total if cap is None else cap
    stride = cap + pad
    got = c_uint64(0)
    with Bufs(dev) as b:
        pos = b.alloc(pos_bytes * (cap + GUARD), 0x5A) if want_pos else None
        if entry == "wide":
            assert W == 2
            hi, lo = b.alloc(8 * (cap + GUARD), 0x5A), b.alloc(8 * (cap + GUARD), 0x5A)
            rc = L.kman_extract_wide(dev.ctx, P(p.codes.ptr), p.n_bases, k, flags | (N.KMAN_WANT_POS if want_pos else 0),
                                     P(hi.ptr), P(lo.ptr), P(pos.ptr) if pos else None, pos_bytes, cap, byref(got))
            planes = [dev.download(x, cap + GUARD, np.uint64) for x in (hi, lo)]
        else:
            words = b.alloc(8 * (W * stride + GUARD), 0x5A)
            rc = L.kman_extract_words(dev.ctx, P(p.codes.ptr), p.n_bases, k, flags, P(words.ptr), stride,
                                      P(pos.ptr) if pos else None, pos_bytes, cap, byref(got))
            flat = dev.download(words, W * stride + GUARD, np.uint64)
            planes = [flat[j * stride:(j + 1) * stride] for j in range(W)]
            planes[-1] = flat[(W - 1) * stride:]  # (with the guard after the last plane)
        n = int(got.value)
        # rows that may have been written: all n, or on KMAN_ECAP at most cap (kman_extract_words: none)
        m = n if rc == N.KMAN_OK else (cap if entry == "wide" else 0)
        clean = all(_untouched(x[m:]) for x in planes)
        rows = np.stack([x[:m] for x in planes], axis=1) if m else np.zeros((0, W), np.uint64)
        hp = None
        if pos:
            hp = dev.download(pos, cap + GUARD, np.uint32 if pos_bytes == 4 else np.uint64)
            clean = clean and _untouched(hp[m:])
            hp = hp[:m]
    return rc, n, rows, hp, clean


def _check_extract(dev, recs, k, flag_list=None, entries=None):
    from kman_amd import engine

    N = _N()
    refs = _refs(recs, k)
    p = engine.parse(dev, wc.fasta(recs))
    try:
        assert p.n_bases == sum(len(s) for _, s in recs)
        assert [int(x) for x in p.rec_seq] == wc.rec_starts(recs)
        for flags in flag_list or (0, N.KMAN_RC, N.KMAN_CANONICAL):
            want_rows, want_pos = refs[N.KMAN_CANONICAL if flags & N.KMAN_CANONICAL else flags]
            got = {}
            for entry in entries or (("wide", "words") if k <= 64 else ("words",)):
                rc, n, rows, pos, clean = _extract(dev, p, k, flags, entry, len(want_rows))
                assert rc == N.KMAN_OK, (entry, flags, N.lib().kman_last_error(dev.ctx))
                assert n == len(want_rows), (entry, flags)
                assert np.array_equal(rows, want_rows), (entry, flags)
                assert np.array_equal(pos, want_pos), (entry, flags)
                assert clean, (entry, flags)
                got[entry] = rows
            if len(got) == 2:  # plane 0 / 1 of the word kernel == hi / lo of the rolled one
                assert got["wide"].tobytes() == got["words"].tobytes()
    finally:
        p.free()
    return refs


@pytest.mark.parametrize("k", KS + KS_LONG)
def test_extract_lengths(dev, k):
    N = _N()
    for n in wc.lengths(k):
        refs = _check_extract(dev, [(b"s%d" % n, wc.clean(n, k))], k,
                              (0, N.KMAN_RC, N.KMAN_CANONICAL, N.KMAN_RC | N.KMAN_CANONICAL))
        assert len(refs[0][0]) == max(0, n - k + 1)


@pytest.mark.parametrize("kind", ["N", "record"])
@pytest.mark.parametrize("k", KS + KS_LONG)
def test_extract_events_at_tile_edges(dev, k, kind):
    for at in wc.event_offsets(k):
        _check_extract(dev, wc.with_n(at, k) if kind == "N" else wc.with_start(at, k), k)
    for first in (wc.TILE - 40, 2 * wc.TILE - k - 1):
        none = _check_extract(dev, wc.two_events(k, k - 1, first, kind == "record", k), k)
        one = _check_extract(dev, wc.two_events(k, k, first, kind == "record", k), k)

        def between(refs, e):  # windows from after the first event that end before base e
            return [int(x) >> 1 for x in refs[0][1] if first < int(x) >> 1 and (int(x) >> 1) + k <= e]

        assert between(none, first + k) == []
        assert between(one, first + k + 1) == [first + 1]


@pytest.mark.parametrize("k", KS + KS_LONG)
def test_extract_built_keys(dev, k):
    N = _N()
    ats = (wc.TILE - 3, wc.TILE - k, 2 * wc.TILE - 1, 2 * wc.TILE)
    built = [b"A" * k, b"T" * k]
    if k % 2 == 0:
        built.append(wc.palindrome(k))
    if k < 64:
        built += [wc.hi_tie(k, True), wc.hi_tie(k, False)]
    for i, w in enumerate(built):
        for at in ats:
            refs = _check_extract(dev, wc.embed(w, at, (k, i)), k)
            rows, pos = refs[N.KMAN_CANONICAL]
            j = int(np.nonzero(pos == np.uint64(at << 1))[0][0])
            canon = min(w, wc.revcomp(w))
            assert tuple(int(x) for x in rows[j]) == wc.to_words(canon)
            frows, fpos = refs[0]
            assert tuple(int(x) for x in frows[j]) == wc.to_words(w)
    if k == 64:  # the key T x 64 is the words (~0, ~0)
        refs = _check_extract(dev, [(b"t", b"T" * (wc.TILE + 70))], k)
        assert (refs[0][0] == np.uint64(wc.ONES)).all()
        _check_extract(dev, [(b"t", wc.clean(wc.TILE - 64, 1) + b"T" * 64), (b"u", b"T" * 64 + wc.clean(9, 2))], k)


@pytest.mark.parametrize("k", KS)
def test_extract_outputs(dev, k):
    """pos widths, no pos, count-only calls, KMAN_ECAP and strides."""
    from kman_amd import engine

    N = _N()
    L = N.lib()
    recs = wc.with_n(wc.TILE + 1, k) + [(b"tail", wc.clean(k + 3, "tail"))]
    refs = _refs(recs, k)
    p = engine.parse(dev, wc.fasta(recs))
    try:
        for flags in (0, N.KMAN_RC, N.KMAN_CANONICAL):
            want_rows, want_pos = refs[flags]
            total = len(want_rows)
            assert want_pos.max() < 1 << 32
            for entry in ("wide", "words"):
                # u32 pos
                rc, n, rows, pos, clean = _extract(dev, p, k, flags, entry, total, pos_bytes=4)
                assert (rc, n) == (N.KMAN_OK, total) and clean
                assert pos.dtype == np.uint32 and np.array_equal(pos.astype(np.uint64), want_pos)
                assert np.array_equal(rows, want_rows)
                # keys only
                rc, n, rows, pos, clean = _extract(dev, p, k, flags, entry, total, want_pos=False)
                assert (rc, n) == (N.KMAN_OK, total) and clean and pos is None
                assert np.array_equal(rows, want_rows)
                # one row short: KMAN_ECAP with the total, nothing past cap
                for pb in (4, 8):
                    rc, n, rows, pos, clean = _extract(dev, p, k, flags, entry, total, pos_bytes=pb, cap=total - 1)
                    assert (rc, n) == (N.KMAN_ECAP, total) and clean
                    if entry == "wide":  # (it writes the rows that fit)
                        assert np.array_equal(rows, want_rows[:total - 1])
                        assert np.array_equal(pos.astype(np.uint64), want_pos[:total - 1])
            # planes further apart than cap: the gap stays as it was
            rc, n, rows, pos, clean = _extract(dev, p, k, flags, "words", total, pad=5)
            assert (rc, n) == (N.KMAN_OK, total) and clean
            assert np.array_equal(rows, want_rows) and np.array_equal(pos, want_pos)
            # count only
            got = c_uint64(0)
            assert L.kman_extract_wide(dev.ctx, P(p.codes.ptr), p.n_bases, k, flags, None, None, None, 0, 0,
                                       byref(got)) == N.KMAN_OK
            assert got.value == total
            got = c_uint64(0)
            assert L.kman_extract_words(dev.ctx, P(p.codes.ptr), p.n_bases, k, flags, None, 0, None, 0, 0,
                                        byref(got)) == N.KMAN_OK
            assert got.value == total
            assert engine.count_kmers(p, k, bool(flags & N.KMAN_RC), bool(flags & N.KMAN_CANONICAL)) == total
    finally:
        p.free()


def test_count_only_agrees_with_count_kmers(dev):
    """kman_count_kmers takes k <= 32 only (one 64-bit key); there it and the
    count-only call of kman_extract_words agree with the reference, and the
    wide kernel's count-only call continues the same series at k = 33."""
    from kman_amd import engine

    N = _N()
    L = N.lib()
    recs = wc.with_n(wc.TILE - 1, "ck") + wc.with_start(2 * wc.TILE + 7, "ck2")
    p = engine.parse(dev, wc.fasta(recs))
    try:
        for k in (31, 32, 33):
            for flags in (0, N.KMAN_RC, N.KMAN_CANONICAL):
                want = len(wc.windows(recs, k, bool(flags & N.KMAN_RC), bool(flags & N.KMAN_CANONICAL)))
                got = c_uint64(0)
                assert L.kman_extract_words(dev.ctx, P(p.codes.ptr), p.n_bases, k, flags, None, 0, None, 0, 0,
                                            byref(got)) == N.KMAN_OK
                assert got.value == want
                got = c_uint64(0)
                if k <= 32:
                    assert L.kman_count_kmers(dev.ctx, P(p.codes.ptr), p.n_bases, k, flags, byref(got)) == N.KMAN_OK
                else:
                    assert L.kman_extract_wide(dev.ctx, P(p.codes.ptr), p.n_bases, k, flags, None, None, None, 0, 0,
                                               byref(got)) == N.KMAN_OK
                assert got.value == want
    finally:
        p.free()


def test_extract_refusals(dev):
    from kman_amd import engine

    N = _N()
    L = N.lib()
    p = engine.parse(dev, wc.fasta([(b"s", wc.clean(300, "ref"))]))
    try:
        with Bufs(dev) as b:
            hi, lo, pos = b.alloc(8 * 400, 0x5A), b.alloc(8 * 400, 0x5A), b.alloc(8 * 400, 0x5A)
            got = c_uint64(0)
            codes = P(p.codes.ptr)

            def wide(k=40, flags=N.KMAN_WANT_POS, hi_=hi.ptr, lo_=lo.ptr, pb=8, codes_=codes):
                return L.kman_extract_wide(dev.ctx, codes_, p.n_bases, k, flags, P(hi_), P(lo_), P(pos.ptr), pb, 400,
                                           byref(got))

            assert wide() == N.KMAN_OK and got.value == 261
            assert wide(k=32) == N.KMAN_EINVAL
            assert wide(k=65) == N.KMAN_EINVAL
            assert wide(lo_=None) == N.KMAN_EINVAL
            assert wide(hi_=None) == N.KMAN_EINVAL
            assert wide(pb=2) == N.KMAN_EINVAL
            assert wide(codes_=P(p.codes.ptr + 8)) == N.KMAN_EINVAL

            def words(k=20, stride=400, cap=400, pb=8):
                return L.kman_extract_words(dev.ctx, codes, p.n_bases, k, 0, P(hi.ptr), stride, P(pos.ptr), pb, cap,
                                            byref(got))

            # (one plane fits hi: W = 1 at k = 20)
            assert words(k=20) == N.KMAN_OK and got.value == 281
            assert words(k=1) == N.KMAN_EINVAL
            assert words(k=20, pb=2) == N.KMAN_EINVAL
            assert words(k=20, stride=399) == N.KMAN_EINVAL
            dev.sync()
            # a refused call writes nothing
            dev.memset(hi, 0x5A, 8 * 400)
            assert words(k=20, stride=399) == N.KMAN_EINVAL and wide(k=65) == N.KMAN_EINVAL
            assert _untouched(dev.download(hi, 400, np.uint64))
    finally:
        p.free()


def test_extract_three_calls_one_context(dev):
    """The look-back status words are reused across calls by epoch: a short
    call between two long ones must not disturb either."""
    N = _N()
    k = 48
    for recs in (wc.with_n(wc.TILE, "c1"), [(b"one", wc.clean(wc.TILE, "c2"))], wc.with_start(2 * wc.TILE - 1, "c3")):
        _check_extract(dev, recs, k, (N.KMAN_RC,))


# ================================================================ run-length
def _vals(n, vb):
    i = np.arange(n, dtype=np.uint64)
    v = i * np.uint64(0x9E3779B97F4A7C15) + np.uint64(0x8000000000000001)
    return v.astype(np.uint32) if vb == 4 else v


def _rle(dev, entry, mode, rows, vals, vb, ovb, pad=0):
    """-> (rc, n_out, out rows (m, W), out vals (m,), guard untouched)."""
    N = _N()
    L = N.lib()
    n, W = rows.shape
    stride = n + pad
    m_code = N.KMAN_FINISH_UNIQ if mode == "uniq" else N.KMAN_FINISH_COUNT
    out = c_uint64(0)
    with Bufs(dev) as b:
        dv = b.put(vals) if vals is not None else None
        dov = b.alloc(ovb * (n + GUARD), 0x5A)
        if entry == "wide":
            assert W == 2 and vb == ovb and pad == 0
            hi, lo = b.put(rows[:, 0]), b.put(rows[:, 1])
            ohi, olo = b.alloc(8 * (n + GUARD), 0x5A), b.alloc(8 * (n + GUARD), 0x5A)
            rc = L.kman_rle_wide(dev.ctx, m_code, P(hi.ptr), P(lo.ptr), P(dv.ptr) if dv else None, vb, n, P(ohi.ptr),
                                 P(olo.ptr), P(dov.ptr), byref(out))
            dev.sync()
            planes = [dev.download(x, n + GUARD, np.uint64) for x in (ohi, olo)]
        else:
            flat = np.full(W * stride + 1, 0xA5A5A5A5A5A5A5A5, np.uint64)
            for j in range(W):
                flat[j * stride:j * stride + n] = rows[:, j]
            dw = b.put(flat)
            ow = b.alloc(8 * (W * stride + GUARD), 0x5A)
            rc = L.kman_rle_words(dev.ctx, m_code, P(dw.ptr), W, stride, P(dv.ptr) if dv else None, vb, n, P(ow.ptr),
                                  stride, P(dov.ptr), ovb, byref(out))
            dev.sync()
            f = dev.download(ow, W * stride + GUARD, np.uint64)
            planes = [f[j * stride:(j + 1) * stride] for j in range(W)]
            planes[-1] = f[(W - 1) * stride:]
        m = int(out.value)
        ov = dev.download(dov, n + GUARD, np.uint32 if ovb == 4 else np.uint64)
        clean = all(_untouched(x[m:]) for x in planes) and _untouched(ov[m:])
        orow = np.stack([x[:m] for x in planes], axis=1) if m else np.zeros((0, W), np.uint64)
    return rc, m, orow, ov[:m], clean


def _check_rle(dev, rows_list, W, wide=True):
    """Both modes and every value width of both entry points on one row list."""
    N = _N()
    n = len(rows_list)
    rows = np.array(rows_list, dtype=np.uint64).reshape(n, W)
    v8 = _vals(n, 8)
    want = {}
    for mode in ("count", "uniq"):
        keys, out = wc.rle(rows_list, [int(x) for x in v8], mode)
        want[mode] = (np.array(keys, dtype=np.uint64).reshape(len(keys), W), np.array(out, dtype=np.uint64))
    got2 = {}
    for mode in ("count", "uniq"):
        wk, wv = want[mode]
        for vb in (4, 8):
            for ovb in (4, 8):
                vals = _vals(n, vb) if mode == "uniq" else None
                # uniq: the payload at the width it is read at, stored at the width asked for
                wv_ = wv
                if mode == "uniq":
                    wv_ = wv & np.uint64((1 << (8 * min(vb, ovb))) - 1)
                for pad in (0, 5):
                    rc, m, orow, ov, clean = _rle(dev, "words", mode, rows, vals, vb, ovb, pad)
                    what = ("words", mode, vb, ovb, pad, n, W)
                    assert rc == N.KMAN_OK, what
                    assert m == len(wk), what
                    assert np.array_equal(orow, wk), what
                    assert np.array_equal(ov.astype(np.uint64), wv_), what
                    assert clean, what
                if vb == ovb:
                    got2[(mode, vb)] = (orow, ov)
        if W == 2 and wide:
            for vb in (4, 8):
                vals = _vals(n, vb) if mode == "uniq" else None
                rc, m, orow, ov, clean = _rle(dev, "wide", mode, rows, vals, vb, vb)
                what = ("wide", mode, vb, n)
                assert rc == N.KMAN_OK, what
                assert m == len(wk), what
                assert np.array_equal(orow, wk), what
                wv_ = wv & np.uint64((1 << (8 * vb)) - 1) if mode == "uniq" else wv
                assert np.array_equal(ov.astype(np.uint64), wv_), what
                assert clean, what
                # kman_rle_words at W = 2 gives the same rows and values
                assert orow.tobytes() == got2[(mode, vb)][0].tobytes()
                assert ov.tobytes() == got2[(mode, vb)][1].tobytes()


def _layout_sets(n):
    seen, out = set(), []
    for tile, per in ((wc.RLE_WIDE_TILE, wc.RLE_WIDE_PER), (wc.RLE_WORDS_TILE, wc.RLE_WORDS_PER)):
        for name, sizes in wc.rle_layouts(n, tile, per).items():
            if tuple(sizes) not in seen:
                seen.add(tuple(sizes))
                out.append(("%s/%d" % (name, tile), sizes))
    return out


RLE_N = [0, 1, 2, 15, 16, 17, 2047, 2048, 2049, 4095, 4096, 4097, 3 * 4096 + 1]


@pytest.mark.parametrize("n", RLE_N)
def test_rle_pairs(dev, n):
    """kman_rle_wide and kman_rle_words (W = 2) on every layout."""
    for name, sizes in _layout_sets(n):
        _check_rle(dev, wc.rle_rows(sizes, 2, "all"), 2)
        if name.startswith("singles") or name.startswith("straddle2"):
            for j in range(2):  # neighbours that differ only in hi, only in lo
                _check_rle(dev, wc.rle_rows(sizes, 2, j), 2)
    if n >= 1:
        ones = ["first", "last"] + (["both"] if n >= 3 else [])
        for which in ones:
            _check_rle(dev, wc.rle_rows([1] * n, 2, "all", ones=which), 2)
            if n >= 4:  # the all-ones key next to a group, not only next to singletons
                sizes = [1, 2] + [1] * (n - 6) + [2, 1] if n >= 6 else [1] * n
                _check_rle(dev, wc.rle_rows(sizes, 2, 1, ones=which), 2)


@pytest.mark.parametrize("W", [1, 3, 5])
@pytest.mark.parametrize("n", RLE_N)
def test_rle_words(dev, n, W):
    for name, sizes in _layout_sets(n):
        _check_rle(dev, wc.rle_rows(sizes, W, "all"), W)
        if name.startswith("singles"):
            for j in range(W):  # neighbours that differ in word j only
                _check_rle(dev, wc.rle_rows(sizes, W, j), W)
    if n >= 3:
        _check_rle(dev, wc.rle_rows([1] * n, W, "all", ones="both"), W)


def test_rle_three_calls_one_context(dev):
    for n in (3 * 4096 + 1, 4096, 3 * 4096 + 1, 17):
        sizes = wc.rle_layouts(n, wc.RLE_WIDE_TILE, wc.RLE_WIDE_PER)["long" if n > 4096 else "singles"]
        _check_rle(dev, wc.rle_rows(sizes, 2, "all"), 2)


def test_rle_refusals(dev):
    N = _N()
    L = N.lib()
    n = 100
    rows = np.array(wc.rle_rows([1] * n, 2, "all"), dtype=np.uint64)
    out = c_uint64(0)
    C, U = N.KMAN_FINISH_COUNT, N.KMAN_FINISH_UNIQ
    with Bufs(dev) as b:
        w = b.put(np.ascontiguousarray(rows.T))  # plane-major, stride n
        v = b.put(_vals(n, 8))
        ow, ov = b.alloc(8 * 2 * n, 0x5A), b.alloc(8 * n, 0x5A)
        hi, lo, ohi, olo = w.ptr, w.ptr + 8 * n, ow.ptr, ow.ptr + 8 * n

        def wide(mode=U, hi_=hi, lo_=lo, v_=v.ptr, vb=8, ohi_=ohi, olo_=olo, ov_=ov.ptr, out_=byref(out)):
            return L.kman_rle_wide(dev.ctx, mode, P(hi_), P(lo_), P(v_), vb, n, P(ohi_), P(olo_), P(ov_), out_)

        assert wide() == N.KMAN_OK and out.value == n
        assert wide(mode=C, v_=None) == N.KMAN_OK and out.value == n
        for bad in (N.KMAN_FINISH_SORT, 3, -1):
            assert wide(mode=bad) == N.KMAN_EINVAL
        for vb in (0, 2, 16):
            assert wide(vb=vb) == N.KMAN_EINVAL
        for kw in ({"hi_": None}, {"lo_": None}, {"ohi_": None}, {"olo_": None}, {"ov_": None}, {"v_": None},
                   {"out_": None}):
            assert wide(**kw) == N.KMAN_EINVAL, kw

        def words(mode=U, w_=w.ptr, W=2, stride=n, v_=v.ptr, vb=8, ow_=ow.ptr, ostride=n, ov_=ov.ptr, ovb=8,
                  out_=byref(out)):
            return L.kman_rle_words(dev.ctx, mode, P(w_), W, stride, P(v_), vb, n, P(ow_), ostride, P(ov_), ovb, out_)

        assert words() == N.KMAN_OK and out.value == n
        assert words(mode=C, v_=None, vb=0) == N.KMAN_OK and out.value == n  # (count mode reads no values)
        for bad in (N.KMAN_FINISH_SORT, 3, -1):
            assert words(mode=bad) == N.KMAN_EINVAL
        assert words(W=0) == N.KMAN_EINVAL
        for x in (0, 2, 16):
            assert words(ovb=x) == N.KMAN_EINVAL
            assert words(vb=x) == N.KMAN_EINVAL
        for kw in ({"w_": None}, {"ow_": None}, {"ov_": None}, {"v_": None}, {"out_": None}, {"stride": n - 1},
                   {"ostride": n - 1}):
            assert words(**kw) == N.KMAN_EINVAL, kw
        dev.sync()
        dev.memset(ow, 0x5A, 8 * 2 * n)
        assert words(ostride=n - 1) == N.KMAN_EINVAL and wide(vb=2) == N.KMAN_EINVAL
        assert _untouched(dev.download(ow, 2 * n, np.uint64))


# ========================================================= small device ops
STRIDE1 = 8192 * 256  # elements of one grid stride
OPS_N = [0, 1, 255, 256, 257, STRIDE1, STRIDE1 + 1, 2 * STRIDE1 + 3]


@pytest.mark.parametrize("n", OPS_N)
def test_iota_gather(dev, n):
    N = _N()
    L = N.lib()
    rng = np.random.default_rng(n + 1)
    with Bufs(dev) as b:
        v = b.alloc(8 * (n + GUARD), 0x5A)
        assert L.kman_iota_u64(dev.ctx, P(v.ptr), n) == N.KMAN_OK
        got = dev.download(v, n + GUARD, np.uint64)
        assert np.array_equal(got[:n], np.arange(n, dtype=np.uint64)) and _untouched(got[n:])
        src8 = rng.integers(0, 1 << 64, max(n, 1), dtype=np.uint64)
        src4 = rng.integers(0, 1 << 32, max(n, 1), dtype=np.uint32)
        d8, d4 = b.put(src8), b.put(src4)
        idxs = [rng.permutation(n).astype(np.uint64), np.arange(n, dtype=np.uint64)[::-1].copy(),
                rng.integers(0, max(n, 1), n, dtype=np.uint64) // np.uint64(3)]
        dst = b.alloc(8 * (n + GUARD))
        for idx in idxs:
            di = b.put(idx)
            for src, d, eb, dt in ((src8, d8, 8, np.uint64), (src4, d4, 4, np.uint32)):
                dev.memset(dst, 0x5A, 8 * (n + GUARD))
                assert L.kman_gather(dev.ctx, P(d.ptr), P(di.ptr), n, P(dst.ptr), eb) == N.KMAN_OK
                got = dev.download(dst, n + GUARD, dt)
                assert np.array_equal(got[:n], src[idx]) and _untouched(got[n:])
            di.free()
        for eb in (0, 2, 16):
            assert L.kman_gather(dev.ctx, P(d8.ptr), P(d8.ptr), n, P(dst.ptr), eb) == N.KMAN_EINVAL


@pytest.mark.parametrize("n", OPS_N)
def test_or_widen(dev, n):
    """kman_or_u64: v[i] |= value; kman_widen_u32: out[i] = in[i] | value (the
    source tag of a u32 payload moved into a tagged u64 array)."""
    N = _N()
    L = N.lib()
    rng = np.random.default_rng(n + 2)
    with Bufs(dev) as b:
        a = rng.integers(0, 1 << 62, n + GUARD, dtype=np.uint64)
        for value in (0, 1 << 63, (0xA5 << 56) | 1):
            v = b.put(a)
            assert L.kman_or_u64(dev.ctx, P(v.ptr), n, value) == N.KMAN_OK
            got = dev.download(v, n + GUARD, np.uint64)
            assert np.array_equal(got[:n], a[:n] | np.uint64(value)) and np.array_equal(got[n:], a[n:])
            v.free()
        a4 = rng.integers(0, 1 << 32, max(n, 1), dtype=np.uint32)
        a4[:1] = 0xFFFFFFFF
        d4 = b.put(a4)
        out = b.alloc(8 * (n + GUARD))
        for value in (0, 1 << 63, 0xFF << 56, 3 << 32):
            dev.memset(out, 0x5A, 8 * (n + GUARD))
            assert L.kman_widen_u32(dev.ctx, P(d4.ptr), P(out.ptr), n, value) == N.KMAN_OK
            got = dev.download(out, n + GUARD, np.uint64)
            assert np.array_equal(got[:n], a4[:n].astype(np.uint64) | np.uint64(value)) and _untouched(got[n:])


@pytest.mark.parametrize("n", OPS_N)
def test_batch_tags(dev, n):
    N = _N()
    L = N.lib()
    rng = np.random.default_rng(n + 3)
    perm = rng.permutation(n).astype(np.uint64)
    with Bufs(dev) as b:
        dp = b.put(perm)
        tags = b.alloc(8 * (n + GUARD))
        for start, per in ((5, 1), (5, 7), (123, n + 1), (1 << 33, 7), (0, 1000)):
            dev.memset(tags, 0x5A, 8 * (n + GUARD))
            assert L.kman_batch_tags(dev.ctx, P(dp.ptr), n, start, per, P(tags.ptr)) == N.KMAN_OK
            got = dev.download(tags, n + GUARD, np.uint64)
            assert np.array_equal(got[:n], (np.uint64(start) + perm) // np.uint64(per)) and _untouched(got[n:])
        assert L.kman_batch_tags(dev.ctx, P(dp.ptr), n, 5, 0, P(tags.ptr)) == N.KMAN_EINVAL
        # kman_tag_batches: the tag above key_bits
        keys = rng.integers(0, 1 << 40, n + GUARD, dtype=np.uint64)
        for bits, first, per in ((40, 0, 1000), (40, 5, 7), (42, 1 << 20, 3)):
            dk = b.put(keys)
            assert L.kman_tag_batches(dev.ctx, P(dk.ptr), n, bits, first, per) == N.KMAN_OK
            got = dev.download(dk, n + GUARD, np.uint64)
            want = keys[:n] | (((np.uint64(first) + np.arange(n, dtype=np.uint64)) // np.uint64(per)) << np.uint64(bits))
            assert np.array_equal(got[:n], want) and np.array_equal(got[n:], keys[n:])
            dk.free()


def test_tag_batches_by_hand(dev):
    N = _N()
    L = N.lib()
    n = 256
    keys = [(i * 0x9E3779B97F4A7C15) & ((1 << 56) - 1) for i in range(n)]
    with Bufs(dev) as b:
        # tags 0..255 need 8 bits: they fit above 56 key bits, not above 57
        dk = b.put(np.array(keys, dtype=np.uint64))
        assert L.kman_tag_batches(dev.ctx, P(dk.ptr), n, 56, 0, 1) == N.KMAN_OK
        got = dev.download(dk, n, np.uint64)
        assert [int(x) for x in got] == [k_ | (i << 56) for i, k_ in enumerate(keys)]
        assert int(got[-1]) >> 63 == 1
        dk2 = b.put(np.array(keys, dtype=np.uint64))
        assert L.kman_tag_batches(dev.ctx, P(dk2.ptr), n, 57, 0, 1) == N.KMAN_EINVAL
        assert L.kman_tag_batches(dev.ctx, P(dk2.ptr), n, 64, 0, 1) == N.KMAN_EINVAL
        assert L.kman_tag_batches(dev.ctx, P(dk2.ptr), n, 40, 0, 0) == N.KMAN_EINVAL
        # first_index counts: items 300.. in batches of 100 are batches 3, 3, .., 4, ..
        assert L.kman_tag_batches(dev.ctx, P(dk2.ptr), n, 60, 300, 100) == N.KMAN_OK
        got = dev.download(dk2, n, np.uint64)
        assert [int(x) for x in got] == [k_ | (((300 + i) // 100) << 60) for i, k_ in enumerate(keys)]


def test_memcpy_d2d_odd(dev):
    N = _N()
    L = N.lib()
    src = np.arange(1000, dtype=np.uint8) * 7 + 1
    with Bufs(dev) as b:
        ds = b.put(src)
        dd = b.alloc(1024, 0x5A)
        assert L.kman_memcpy_d2d(dev.ctx, P(dd.ptr + 5), P(ds.ptr + 3), 777) == N.KMAN_OK
        assert L.kman_memcpy_d2d(dev.ctx, P(dd.ptr + 900), P(ds.ptr), 0) == N.KMAN_OK
        got = dev.download(dd, 1024, np.uint8)
        assert np.array_equal(got[5:782], src[3:780])
        assert _untouched(got[:5]) and _untouched(got[782:])


# ================================================================== writers
FTILE = 512
FB = 32768
FMT_N = 3 * FTILE + 5


def _fmt_rows(k, n, seed):
    return [wc.clean(k, ("fmt", seed, i)) for i in range(n)]


def _planes(rows, k):
    """(W, n) u64 planes of k-mer rows."""
    W = wc.nwords(k)
    return np.ascontiguousarray(np.array([wc.to_words(r) for r in rows], dtype=np.uint64).reshape(len(rows), W).T)


def _dev_text(dev, call, want: bytes) -> bytes:
    """The device writer's text through `call(d_out, cap, used)`, with its
    capacity contract: NULL sizes only, one byte short is KMAN_ECAP with
    nothing past cap, an output off 16-byte alignment is refused."""
    N = _N()
    size = len(want)
    used = c_size_t(0)
    assert call(None, 0, used) == N.KMAN_ECAP
    assert used.value == size
    with Bufs(dev) as b:
        out = b.alloc(size + 256, 0x5A)
        used = c_size_t(0)
        assert call(P(out.ptr), size, used) == N.KMAN_OK
        assert used.value == size
        got = dev.download(out, size + 256, np.uint8)
        assert _untouched(got[size:])
        text = got[:size].tobytes()
        dev.memset(out, 0x5A, size + 256)
        used = c_size_t(0)
        assert call(P(out.ptr), size - 1, used) == N.KMAN_ECAP
        assert used.value == size
        short = dev.download(out, size + 256, np.uint8)
        assert _untouched(short[size - 1:])
        assert call(P(out.ptr + 8), size, used) == N.KMAN_EINVAL
    return text


def _count_values(n, cb, seed):
    rng = np.random.default_rng(seed)
    special = [1, 9, 10, 99, 100, (1 << 32) - 1] + ([1 << 40, (1 << 64) - 1, 1 << 32] if cb == 8 else [])
    c = rng.integers(1, 12, n).astype(np.uint64)
    at = rng.choice(n, 400, replace=False)
    c[at] = np.array([special[i % len(special)] for i in range(400)], dtype=np.uint64)
    c[[0, FTILE - 1, FTILE, n - 1]] = np.array([special[-1], 10, 9, special[-1]], dtype=np.uint64)
    return c.astype(np.uint32 if cb == 4 else np.uint64)


def _check_count(dev, k, rows, counts, entry, lo=0):
    """Host and device count writers on rows[lo:], from arrays of all rows."""
    from kman_amd import engine

    N = _N()
    L = N.lib()
    n, cb = len(rows), counts.dtype.itemsize
    m = n - lo
    want = wc.count_text(rows[lo:], [int(x) for x in counts[lo:]], k)
    planes = _planes(rows, k)
    W = planes.shape[0]
    hc = counts[lo:].copy()
    with Bufs(dev) as b:
        dw, dc = b.put(planes), b.put(counts)
        if entry == "wide":
            assert W == 2
            hi, lo_ = planes[0, lo:].copy(), planes[1, lo:].copy()
            host = engine._format(L.kman_format_count_wide, hi.ctypes.data_as(c_void_p), lo_.ctypes.data_as(c_void_p),
                                  hc.ctypes.data_as(c_void_p), cb, m, k)

            def call(d_out, cap, used):
                return L.kman_format_count_wide_dev(dev.ctx, P(dw.ptr + 8 * lo), P(dw.ptr + 8 * (n + lo)),
                                                    P(dc.ptr + cb * lo), cb, m, k, d_out, cap, byref(used))
        else:
            host = engine._format(L.kman_format_count_words, c_void_p(planes.ctypes.data + 8 * lo), n,
                                  hc.ctypes.data_as(c_void_p), cb, m, k)

            def call(d_out, cap, used):
                return L.kman_format_count_words_dev(dev.ctx, P(dw.ptr + 8 * lo), n, P(dc.ptr + cb * lo), cb, m, k,
                                                     d_out, cap, byref(used))

        assert host == want, (entry, k, cb, lo)
        assert _dev_text(dev, call, want) == want, (entry, k, cb, lo)
    return want


FMT_CASES = [("wide", k) for k in (33, 61, 62, 64)] + [("words", k) for k in (33, 61, 64, 65, 129)]


@pytest.mark.parametrize("cb", [4, 8])
@pytest.mark.parametrize("entry,k", FMT_CASES)
def test_count_writers(dev, entry, k, cb):
    rows = _fmt_rows(k, FMT_N, k)
    rows[0], rows[FTILE] = b"T" * k, b"A" * k
    counts = _count_values(FMT_N, cb, k)
    _check_count(dev, k, rows, counts, entry)
    _check_count(dev, k, rows, counts, entry, lo=700)  # a row slice that starts inside a tile


@pytest.mark.parametrize("cb", [4, 8])
@pytest.mark.parametrize("entry", ["wide", "words"])
def test_count_writers_at_the_lds_limit(dev, entry, cb):
    """k = 61, one-digit counts: a full tile's text is 512 x 64 = 32 768 bytes,
    the largest that is staged in LDS.  One count of 10 in the second tile
    makes that tile 32 769 bytes: written straight to HBM between two staged
    tiles.  k = 62: every full tile is over; k = 33: none is."""
    k = 61
    rows = _fmt_rows(k, FMT_N, "lds")
    dt = np.uint32 if cb == 4 else np.uint64
    ones = (np.arange(FMT_N) % 9 + 1).astype(dt)
    want = _check_count(dev, k, rows, ones, entry)
    assert len(want) == FMT_N * 64 and FTILE * 64 == FB
    for at in (FTILE, FTILE + 255, 2 * FTILE - 1):
        c = ones.copy()
        c[at] = 10
        want = _check_count(dev, k, rows, c, entry)
        assert len(want) == FMT_N * 64 + 1
    c = ones.copy()
    c[[0, FTILE, 2 * FTILE]] = 10  # every full tile one byte over
    _check_count(dev, k, rows, c, entry)
    c = ones.copy()
    c[[0, 2 * FTILE, 3 * FTILE]] = 10  # only the middle tile staged
    _check_count(dev, k, rows, c, entry)
    for k2 in (62, 33):
        rows2 = _fmt_rows(k2, FMT_N, "lds%d" % k2)
        want = _check_count(dev, k2, rows2, ones, entry)
        assert (FTILE * (k2 + 3) > FB) == (k2 == 62)


@pytest.mark.parametrize("name_len", [0, 3, 1500])
@pytest.mark.parametrize("pb", [4, 8])
@pytest.mark.parametrize("entry,k", FMT_CASES)
def test_uniq_writers(dev, entry, k, pb, name_len):
    """u64 positions put record starts past 2^32; names of 1500 bytes push a
    tile's text past the LDS buffer."""
    from kman_amd import engine

    N = _N()
    L = N.lib()
    rng = np.random.default_rng(k * 100 + pb + name_len)
    R = 37
    span = (1 << 34) if pb == 8 else (1 << 30)
    rec_seq = np.concatenate([[0], np.sort(rng.choice(span // 2, R - 1, replace=False))]).astype(np.uint64)
    names = [(b"r%d" % i + b"\tx" * (name_len // 2))[:name_len] for i in range(R)]
    assert all(len(x) == name_len for x in names)
    blob = b"".join(names)
    name_off = np.zeros(R + 1, np.uint64)
    name_off[1:] = np.cumsum([len(x) for x in names])
    n = FMT_N
    rows = _fmt_rows(k, n, ("u", k))
    g = rng.integers(0, span // 2, n, dtype=np.uint64)
    g[:R] = rec_seq  # the first base of every record
    strand = rng.integers(0, 2, n, dtype=np.uint64)
    strand[:4] = [0, 1, 0, 1]
    pos64 = (g << np.uint64(1)) | strand
    pos = pos64.astype(np.uint32 if pb == 4 else np.uint64)
    assert pb == 4 or int(rec_seq[-1]) > 1 << 32
    planes = _planes(rows, k)
    hnames = (blob + b"\0")
    for lo in (0, 700):
        m = n - lo
        want = wc.uniq_text(rows[lo:], [int(x) for x in pos64[lo:]], k, names, [int(x) for x in rec_seq])
        hp = pos[lo:].copy()
        with Bufs(dev) as b:
            dw, dp = b.put(planes), b.put(pos)
            dn, do, dr = b.put(np.frombuffer(hnames, np.uint8)), b.put(name_off), b.put(rec_seq)
            if entry == "wide":
                hi, lo_ = planes[0, lo:].copy(), planes[1, lo:].copy()
                host = engine._format(L.kman_format_uniq_wide, hi.ctypes.data_as(c_void_p),
                                      lo_.ctypes.data_as(c_void_p), hp.ctypes.data_as(c_void_p), pb, m, k, hnames,
                                      name_off.ctypes.data_as(c_void_p), rec_seq.ctypes.data_as(c_void_p), R)

                def call(d_out, cap, used):
                    return L.kman_format_uniq_wide_dev(dev.ctx, P(dw.ptr + 8 * lo), P(dw.ptr + 8 * (n + lo)),
                                                       P(dp.ptr + pb * lo), pb, m, k, P(dn.ptr), P(do.ptr), P(dr.ptr),
                                                       R, d_out, cap, byref(used))
            else:
                host = engine._format(L.kman_format_uniq_words, c_void_p(planes.ctypes.data + 8 * lo), n,
                                      hp.ctypes.data_as(c_void_p), pb, m, k, hnames,
                                      name_off.ctypes.data_as(c_void_p), rec_seq.ctypes.data_as(c_void_p), R)

                def call(d_out, cap, used):
                    return L.kman_format_uniq_words_dev(dev.ctx, P(dw.ptr + 8 * lo), n, P(dp.ptr + pb * lo), pb, m, k,
                                                        P(dn.ptr), P(do.ptr), P(dr.ptr), R, d_out, cap, byref(used))

            assert host == want, (entry, k, pb, name_len, lo)
            assert _dev_text(dev, call, want) == want, (entry, k, pb, name_len, lo)


def test_writer_refusals(dev):
    N = _N()
    L = N.lib()
    used = c_size_t(0)
    a = np.zeros(8, np.uint64)
    pa = a.ctypes.data_as(c_void_p)
    with Bufs(dev) as b:
        d = b.put(a)
        out = b.alloc(4096, 0x5A)
        for k in (32, 65):
            assert L.kman_format_count_wide(pa, pa, pa, 8, 4, k, None, 0, byref(used), 1) == N.KMAN_EINVAL
            assert L.kman_format_count_wide_dev(dev.ctx, P(d.ptr), P(d.ptr), P(d.ptr), 8, 4, k, P(out.ptr), 4096,
                                                byref(used)) == N.KMAN_EINVAL
            assert L.kman_format_uniq_wide_dev(dev.ctx, P(d.ptr), P(d.ptr), P(d.ptr), 8, 4, k, P(d.ptr), P(d.ptr),
                                               P(d.ptr), 1, P(out.ptr), 4096, byref(used)) == N.KMAN_EINVAL
        assert L.kman_format_count_wide_dev(dev.ctx, P(d.ptr), P(d.ptr), P(d.ptr), 2, 4, 40, P(out.ptr), 4096,
                                            byref(used)) == N.KMAN_EINVAL
        assert L.kman_format_count_words_dev(dev.ctx, P(d.ptr), 3, P(d.ptr), 8, 4, 40, P(out.ptr), 4096,
                                             byref(used)) == N.KMAN_EINVAL  # stride below n
        assert L.kman_format_count_words_dev(dev.ctx, P(d.ptr), 4, P(d.ptr), 8, 4, 1, P(out.ptr), 4096,
                                             byref(used)) == N.KMAN_EINVAL
        assert _untouched(dev.download(out, 4096, np.uint8))


# ==================================================== the documented recipe
@pytest.mark.parametrize("mode", ["count", "uniq"])
@pytest.mark.parametrize("k", [40, 64])
def test_documented_wide_pipeline(dev, k, mode):
    """INTEGRATION.md, "k in 33..64", call by call through the C ABI:
    kman_extract_wide, a stable kman_sort by lo carrying a kman_iota_u64
    index, kman_gather of hi through it, a stable kman_sort by hi over
    2 (k - 32) bits, kman_gather of hi / lo / pos through the final index,
    kman_rle_wide, kman_format_*_wide_dev."""
    import inputs
    from kman_amd import engine

    N = _N()
    L = N.lib()
    text = inputs.messy_records(k, n_records=20, max_len=5000)
    uniq = mode == "uniq"
    p = engine.parse(dev, text)
    nm = engine.DeviceNames(p)
    try:
        with Bufs(dev) as b:
            got = c_uint64(0)
            assert L.kman_extract_wide(dev.ctx, P(p.codes.ptr), p.n_bases, k, 0, None, None, None, 0, 0,
                                       byref(got)) == N.KMAN_OK
            n = int(got.value)
            assert n > 1000
            hi, lo, pos = (b.alloc(8 * n) for _ in range(3))
            flags = N.KMAN_WANT_POS if uniq else 0
            assert L.kman_extract_wide(dev.ctx, P(p.codes.ptr), p.n_bases, k, flags, P(hi.ptr), P(lo.ptr),
                                       P(pos.ptr) if uniq else None, 8, n, byref(got)) == N.KMAN_OK
            assert got.value == n
            perm, key, alt_k, alt_p = (b.alloc(8 * n) for _ in range(4))
            assert L.kman_iota_u64(dev.ctx, P(perm.ptr), n) == N.KMAN_OK
            assert L.kman_memcpy_d2d(dev.ctx, P(key.ptr), P(lo.ptr), 8 * n) == N.KMAN_OK
            in_alt = c_int(0)
            assert L.kman_sort(dev.ctx, P(key.ptr), P(alt_k.ptr), P(perm.ptr), P(alt_p.ptr), 8, n, 64, None,
                               byref(in_alt)) == N.KMAN_OK
            if in_alt.value:
                perm, alt_p = alt_p, perm
            assert L.kman_gather(dev.ctx, P(hi.ptr), P(perm.ptr), n, P(key.ptr), 8) == N.KMAN_OK
            assert L.kman_sort(dev.ctx, P(key.ptr), P(alt_k.ptr), P(perm.ptr), P(alt_p.ptr), 8, n, 2 * (k - 32), None,
                               byref(in_alt)) == N.KMAN_OK
            if in_alt.value:
                perm, alt_p = alt_p, perm
            shi, slo, spos = (b.alloc(8 * n) for _ in range(3))
            for src, dst in ((hi, shi), (lo, slo)) + (((pos, spos),) if uniq else ()):
                assert L.kman_gather(dev.ctx, P(src.ptr), P(perm.ptr), n, P(dst.ptr), 8) == N.KMAN_OK
            vb = 8 if uniq else 4
            ohi, olo, ov = b.alloc(8 * n), b.alloc(8 * n), b.alloc(vb * n)
            assert L.kman_rle_wide(dev.ctx, N.KMAN_FINISH_UNIQ if uniq else N.KMAN_FINISH_COUNT, P(shi.ptr), P(slo.ptr),
                                   P(spos.ptr) if uniq else None, vb, n, P(ohi.ptr), P(olo.ptr), P(ov.ptr),
                                   byref(got)) == N.KMAN_OK
            m = int(got.value)
            assert 0 < m <= n

            def call(d_out, cap, used):
                if uniq:
                    return L.kman_format_uniq_wide_dev(dev.ctx, P(ohi.ptr), P(olo.ptr), P(ov.ptr), vb, m, k,
                                                       P(nm.names.ptr), P(nm.off.ptr), P(nm.rec.ptr), nm.n_records,
                                                       d_out, cap, byref(used))
                return L.kman_format_count_wide_dev(dev.ctx, P(ohi.ptr), P(olo.ptr), P(ov.ptr), vb, m, k, d_out, cap,
                                                    byref(used))

            want = wc.restate(text, k, mode)
            assert _dev_text(dev, call, want) == want
    finally:
        nm.free()
        p.free()
    assert (engine.uniq_text if uniq else engine.count_text)(text, k, dev=dev) == want
