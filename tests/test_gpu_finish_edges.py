"""kman_finish (kman_amd/csrc/segsort.hip) at the edges of its chunk geometry.

tests/finish_cases.py constructs prefix-sorted inputs whose segments sit at
the kernel's thresholds -- 768 | 769 keys and 22 | 23 | 51 | 52 low bits
between the sort paths, lo_bit == 0 and == key_bits, the end of the last
owned segment at the chunk end, among the keys loaded up front, in the further
rounds and one past the staging area, big segments against chunk boundaries,
groups across chunk ends inside presorted slices -- and
tests/test_finish_cases_cpu.py proves that every layout has its property.
Here every entry goes through kman_finish by ctypes: SORT with no, a 4-byte
and an 8-byte payload, COUNT with 4- and 8-byte counts, UNIQ with both
payloads.  Every key, payload, count and n_out equals np_oracle's on the same
keys; 4 KiB of 0xA5 before and after keys, vals, okeys and ovals are intact,
and the output rows past n_out untouched.  The number of "finish" launches (1,
or 2 through the big-segment fallback) is the plan's.  The whole table runs
once more in a child process under KMAN_RANK=ballot (the ranking without LDS
atomics, read at kman_create); the parent compares the child's arrays."""

from __future__ import annotations

import functools
import os
import subprocess
import sys
from ctypes import byref, c_double, c_uint64, c_void_p

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if __name__ == "__main__":  # the child: no conftest
    sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import finish_cases as F  # noqa: E402

pytestmark = pytest.mark.gpu

GUARD = 4096
VARIANTS = (("sort", 0), ("sort", 4), ("sort", 8), ("count", 4), ("count", 8), ("uniq", 4), ("uniq", 8))


def payload(n, vb):
    """u32: arange(n); u64: arange(n) * 3 + 2^40 -- a truncated or misplaced one cannot pass"""
    if vb == 4:
        return np.arange(n, dtype=np.uint32)
    return np.arange(n, dtype=np.uint64) * np.uint64(3) + np.uint64(1 << 40)


class Bench:
    """Guarded device buffers for the largest layout, reused by every call:
    [GUARD | data | GUARD] with the guards (and the outputs) 0xA5 before the
    call.  The data of a call ends exactly at its rear guard."""

    NAMES = ("keys", "alt", "vals", "valt", "okeys", "ovals")

    def __init__(self, dev, cap):
        self.dev = dev
        self.buf = {nm: dev.alloc(8 * cap + 2 * GUARD) for nm in self.NAMES}

    def free(self):
        for b in self.buf.values():
            b.free()

    def _put(self, nm, data, nbytes):
        b = self.buf[nm]
        self.dev.memset(b, 0xA5, nbytes + 2 * GUARD)
        if data is not None:
            self.dev.upload(b, data, GUARD)

    def _get(self, nm, nbytes, dtype):
        """the data region; asserts both guards"""
        raw = self.dev.download(self.buf[nm], nbytes + 2 * GUARD, np.uint8)
        assert (raw[:GUARD] == 0xA5).all(), "wrote before " + nm
        assert (raw[GUARD + nbytes:] == 0xA5).all(), "wrote past " + nm
        return raw[GUARD:GUARD + nbytes].view(dtype)

    def run(self, case, mode, vb):
        """kman_finish on the case's keys -> (launches, n_out, keys, vals)."""
        from kman_amd import _native as N

        L = N.lib()
        keys = F.keys_of(case)
        n = len(keys)
        m = {"sort": N.KMAN_FINISH_SORT, "count": N.KMAN_FINISH_COUNT, "uniq": N.KMAN_FINISH_UNIQ}[mode]
        in_vb = 0 if mode == "count" else vb
        self._put("keys", keys, 8 * n)
        self._put("alt", None, 8 * n)
        self._put("vals", payload(n, in_vb) if in_vb else None, in_vb * n)
        self._put("valt", None, in_vb * n)
        self._put("okeys", None, 8 * n)
        self._put("ovals", None, vb * n)

        def p(nm, on=True):
            return c_void_p(self.buf[nm].ptr + GUARD if on else None)

        out, nl, ms = c_uint64(0), c_uint64(0), c_double(0)
        assert L.kman_timing_enable(self.dev.ctx, 1) == N.KMAN_OK
        try:
            rc = L.kman_finish(self.dev.ctx, p("keys"), p("alt"), p("vals", in_vb), p("valt", in_vb), in_vb, n,
                               case.key_bits, case.lo_bit, m, p("okeys", mode != "sort"),
                               p("ovals", mode != "sort"), 0 if mode == "sort" else vb, byref(out))
            N.check(self.dev.ctx, rc, "kman_finish")
            assert L.kman_timing_query(self.dev.ctx, b"finish", byref(nl), byref(ms)) == N.KMAN_OK
        finally:
            L.kman_timing_enable(self.dev.ctx, 0)
        n_out = int(out.value)
        dt = np.uint32 if vb == 4 else np.uint64
        gk = self._get("keys", 8 * n, np.uint64)
        gv = self._get("vals", in_vb * n, dt) if in_vb else None
        self._get("alt", 8 * n, np.uint8)
        self._get("valt", in_vb * n, np.uint8)
        ok = self._get("okeys", 8 * n, np.uint64)
        ov = self._get("ovals", vb * n, dt) if vb else None
        if mode == "sort":
            assert (ok.view(np.uint8) == 0xA5).all() and (ov is None or (ov.view(np.uint8) == 0xA5).all())
            return int(nl.value), n_out, gk, gv
        assert n_out <= n
        assert (ok[n_out:].view(np.uint8) == 0xA5).all(), "okeys past n_out touched"
        assert (ov[n_out:].view(np.uint8) == 0xA5).all(), "ovals past n_out touched"
        return int(nl.value), n_out, ok[:n_out], ov[:n_out]


@functools.lru_cache(maxsize=None)
def _want(name):
    """np_oracle's answer on the case's keys, in 64-bit integers (shared, read-only)."""
    import np_oracle

    keys = F.keys_of(F.BY_NAME[name])
    sk, order = np_oracle.stable_sort(keys, np.arange(len(keys), dtype=np.int64))
    ck, cc = np_oracle.rle_count(sk)
    uk, upos = np_oracle.rle_uniq(sk, order)
    for a in (sk, order, ck, cc, uk, upos):
        a.setflags(write=False)
    return sk, order, ck, cc, uk, upos


def check(case, mode, vb, got):
    launches, n_out, gk, gv = got
    sk, order, ck, cc, uk, upos = _want(case.name)
    tag = "%s %s%d" % (case.name, mode, vb)
    assert launches == case.launches, "%s: %d finish launches" % (tag, launches)
    if mode == "sort":
        assert n_out == case.n, tag
        np.testing.assert_array_equal(gk, sk, err_msg=tag)
        if vb:
            np.testing.assert_array_equal(gv, payload(case.n, vb)[order], err_msg=tag)
    elif mode == "count":
        assert n_out == len(ck), tag
        np.testing.assert_array_equal(gk, ck, err_msg=tag)
        np.testing.assert_array_equal(gv.astype(np.uint64), cc, err_msg=tag)
    else:
        assert n_out == len(uk), tag
        np.testing.assert_array_equal(gk, uk, err_msg=tag)
        np.testing.assert_array_equal(gv, payload(case.n, vb)[upos], err_msg=tag)


@pytest.fixture(scope="module")
def dev():
    from kman_amd import engine

    return engine.default_device()


@pytest.fixture(scope="module")
def bench(dev):
    b = Bench(dev, max(c.n for c in F.CASES))
    yield b
    b.free()


@pytest.mark.parametrize("fam", F.FAMILIES)
def test_family_matches_oracle(bench, fam):
    for case in F.family(fam):
        for mode, vb in VARIANTS:
            check(case, mode, vb, bench.run(case, mode, vb))


def _kmers(dev, keys, k, pos):
    from kman_amd import engine

    n = len(keys)
    km = engine.Kmers(dev.alloc(8 * n), dev.alloc(8 * n), dev.alloc(4 * n) if pos else None,
                      dev.alloc(4 * n) if pos else None, 4 if pos else 0, n, k, dev.alloc(8 * 256 * 8),
                      lo_bit=engine.split_bits(n, 2 * k))
    dev.upload(km.keys, keys)
    if pos:
        dev.upload(km.pos, np.arange(n, dtype=np.uint32))
    return km


def test_engine_sort_where_split_bits_is_zero(dev):
    """40,000 random 3-mers: split_bits(40000, 6) == 0, so engine.sort,
    rle_count and rle_uniq reach kman_finish with no low bits at all."""
    import np_oracle
    from kman_amd import engine

    n, k = 40_000, 3
    assert engine.split_bits(n, 2 * k) == 0
    rng = np.random.default_rng(40_000)
    keys = rng.integers(0, 1 << (2 * k), size=n, dtype=np.uint64)
    wk, wp = np_oracle.stable_sort(keys, np.arange(n, dtype=np.uint32))
    km = _kmers(dev, keys, k, True)
    try:
        engine.sort(km, dev)
        np.testing.assert_array_equal(dev.download(km.keys, n, np.uint64), wk)
        np.testing.assert_array_equal(dev.download(km.pos, n, np.uint32), wp)
    finally:
        km.free()
    # one key that occurs once among them: 64 values, 63 in use by the crowd
    keys = rng.integers(0, 63, size=n, dtype=np.uint64)
    keys[12_345] = 63
    wk, wp = np_oracle.stable_sort(keys, np.arange(n, dtype=np.uint32))
    km = _kmers(dev, keys, k, False)
    try:
        r = engine.rle_count(km, dev)
        try:
            gk, gc = engine.download_count(dev, r)
        finally:
            engine.free_result(r)
    finally:
        km.free()
    ck, cc = np_oracle.rle_count(wk)
    np.testing.assert_array_equal(gk, ck)
    np.testing.assert_array_equal(gc.astype(np.uint64), cc)
    km = _kmers(dev, keys, k, True)
    try:
        r = engine.rle_uniq(km, dev)
        try:
            gk, gp = engine.download_uniq(dev, r)
        finally:
            engine.free_result(r)
    finally:
        km.free()
    uk, up = np_oracle.rle_uniq(wk, wp)
    assert uk.tolist() == [63] and up.tolist() == [12_345]
    np.testing.assert_array_equal(gk, uk)
    np.testing.assert_array_equal(gp, up)


# ---------------------------------------------------------------- the ballot ranking


def _child(out_path):
    """Every case and variant on a fresh context, concatenated per variant."""
    from kman_amd import engine

    assert os.environ.get("KMAN_RANK") == "ballot"
    dev = engine.Device(0)
    b = Bench(dev, max(c.n for c in F.CASES))
    res = {}
    try:
        for mode, vb in VARIANTS:
            meta, ks, vs = [], [], []
            for case in F.CASES:
                launches, n_out, gk, gv = b.run(case, mode, vb)
                meta.append((launches, n_out, len(gk)))
                ks.append(gk.copy())
                if gv is not None:
                    vs.append(gv.copy())
            res["%s%d_meta" % (mode, vb)] = np.array(meta, dtype=np.int64)
            res["%s%d_k" % (mode, vb)] = np.concatenate(ks)
            if vs:
                res["%s%d_v" % (mode, vb)] = np.concatenate(vs)
    finally:
        b.free()
        dev.close()
    np.savez(out_path, **res)


def test_ballot_ranking_matches_oracle(tmp_path):
    out = str(tmp_path / "ballot.npz")
    env = dict(os.environ, KMAN_RANK="ballot")
    subprocess.run([sys.executable, os.path.abspath(__file__), out], env=env, check=True, timeout=300)
    with np.load(out) as z:
        for mode, vb in VARIANTS:
            meta, ks = z["%s%d_meta" % (mode, vb)], z["%s%d_k" % (mode, vb)]
            vs = z["%s%d_v" % (mode, vb)] if "%s%d_v" % (mode, vb) in z.files else None
            assert len(meta) == len(F.CASES)
            at = 0
            for case, (launches, n_out, ln) in zip(F.CASES, meta.tolist()):
                gv = vs[at:at + ln] if vs is not None else None
                check(case, mode, vb, (launches, n_out, ks[at:at + ln], gv))
                at += ln
            assert at == len(ks)


if __name__ == "__main__":
    _child(sys.argv[1])
