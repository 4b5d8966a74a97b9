"""The region path's capacities at exactly full and one item over
(kman_groups; region_extract.hip, region_pass.hip, region_finish.hip).

tests/region_cases.py builds, for each of the three capacities, inputs whose
target region holds cap - 1, cap and cap + 1 items while every other region
stays strictly inside (tests/test_region_cases_cpu.py proves the fills with
np_oracle).  Here kman_groups itself is called through ctypes, so its return
code is seen: up to the capacity KMAN_OK -- the call stayed on the region
path -- with the oracle's k-mer count and bit-exact rows (np_oracle: stable
sort, rle_count / rle_uniq), keys equal to the general path's; one item over
KMAN_EFALLBACK, then a clean call on the same context, and the engine's text
through its other paths equal to the C oracle's.  The work area is exactly the
plan's size; 4 KiB of 0xA5 behind it and behind the W output rows are checked
after every call."""

from __future__ import annotations

import functools
import os
import subprocess
from ctypes import byref, c_uint32, c_uint64, c_void_p

import numpy as np
import pytest

import region_cases as R

pytestmark = pytest.mark.gpu

GUARD = 4096
ENV_KNOBS = ("KMAN_WIDE_ITEMS", "KMAN_PASS_LINE1", "KMAN_NO_REGION", "KMAN_RG_STAMPS")


@pytest.fixture(scope="module")
def dev():
    from kman_amd import engine

    return engine.default_device()


@functools.lru_cache(maxsize=None)
def _want(edge, delta, k, rc, canonical, mode):
    """The oracle's rows of a built input (read-only, shared)."""
    import np_oracle

    c = R.build(edge, delta, k, rc, canonical)
    keys, pos = np_oracle.stream_kmers(np_oracle.parse_fasta(c.text), k, rc=rc, canonical=canonical)
    sk, sp = np_oracle.stable_sort(keys, pos)
    rows = np_oracle.rle_count(sk) if mode == "count" else np_oracle.rle_uniq(sk, sp)
    for a in rows:
        a.setflags(write=False)
    return len(keys), rows


def _assert_fills(c):
    """The input is what the test says it is (from the oracle's stream)."""
    found, others = R.capacity_report(c)
    for (kind, idx, want), got in zip(c.targets, found):
        assert got == ((want, want) if kind == "sub" else want), (kind, idx)
    assert any(want == c.fill for _, _, want in c.targets) and abs(c.fill - c.cap) <= 1
    for most, cap in others:
        assert most < cap
    if c.rc:  # the filler's reverse strand loads bucket 255: these fills, inside too
        edge = "c0_tile" if c.targets[0][0] == "r0" else "c1_chain0"
        assert R.rc_fills(c) == R.RC_FILLS[edge, c.fill - c.cap]
        assert c.plan.W // 512 + 100 < c.fills.fin[-1] and c.fills.r0[255].max() < c.plan.C0
        assert c.fills.sub_hi[-2:].max() < c.plan.C1


def _assert_item_width(c, mode, env):
    """A case meant for the 4-byte count items can take them, and the k = 21
    cases are the 8-byte ones: the pairing says what it runs."""
    narrow = mode == "count" and c.plan.rest <= 32 and "KMAN_WIDE_ITEMS" not in env
    if c.k in (9, NARROW_K) and mode == "count" and "KMAN_WIDE_ITEMS" not in env:
        assert narrow and c.plan.rest <= 32
    if c.k == 21 or "KMAN_WIDE_ITEMS" in env:
        assert not narrow


def _set_env(monkeypatch, env):
    for name in ENV_KNOBS:
        monkeypatch.delenv(name, raising=False)
    monkeypatch.setenv("KMAN_RG_CHECK", "1")
    for name, v in env.items():
        monkeypatch.setenv(name, v)


class _Buffers:
    """Codes, the work area of exactly the plan's size and W output rows,
    each output and the work area followed by GUARD bytes of 0xA5."""

    def __init__(self, dev, c, mode, vb, fill_all=False):
        from kman_amd import _native as N
        from kman_amd import engine

        self.dev, self.c, self.vb = dev, c, vb
        self.m = N.KMAN_FINISH_UNIQ if mode == "uniq" else N.KMAN_FINISH_COUNT
        self.flags = engine.flags_for(c.rc, mode == "uniq", c.canonical)
        pl = R.plan(len(c.text) - 7, c.k, c.rc, mode, c.canonical)
        wb = c_uint64(0)
        assert N.lib().kman_groups_plan(len(c.text) - 7, c.k, self.flags, self.m, byref(wb)) == N.KMAN_OK
        assert wb.value == pl.work_bytes and (pl.C0, pl.C1, pl.B2) == (c.plan.C0, c.plan.C1, c.plan.B2)
        self.wb, self.W = pl.work_bytes, pl.W
        self.p = engine.parse(dev, c.text)
        assert self.p.n_bases == len(c.text) - 7
        self.sizes = (self.wb, 8 * self.W, vb * self.W)
        self.bufs = [dev.alloc(s + GUARD) for s in self.sizes]
        for b, s in zip(self.bufs, self.sizes):
            dev.memset(b, 0xA5, s + GUARD if fill_all else GUARD, 0 if fill_all else s)
        self.work, self.okeys, self.ovals = self.bufs
        assert self.work.ptr % 256 == 0  # (the lines body of pass 1 needs it)

    def args(self, work_bytes=None, codes=True):
        return (self.dev.ctx, c_void_p(self.p.codes.ptr if codes else None), self.p.n_bases, self.c.k, self.flags,
                self.m, c_void_p(self.work.ptr), self.wb if work_bytes is None else work_bytes)

    def outs(self, nk, no):
        return (c_void_p(self.okeys.ptr), c_void_p(self.ovals.ptr), self.vb, byref(nk), byref(no))

    def guards_intact(self):
        for b, s in zip(self.bufs, self.sizes):
            assert (self.dev.download(b, GUARD, np.uint8, offset=s) == 0xA5).all(), "wrote past a buffer"

    def untouched(self):
        for b, s in zip(self.bufs, self.sizes):
            assert (self.dev.download(b, s + GUARD, np.uint8) == 0xA5).all(), "a refused call wrote"

    def rows(self, n):
        return (self.dev.download(self.okeys, n, np.uint64),
                self.dev.download(self.ovals, n, np.uint32 if self.vb == 4 else np.uint64))

    def free(self):
        for b in self.bufs:
            b.free()
        self.p.free()


def _call(dev, c, mode, vb, cuts=None):
    """kman_groups (or its three-call form with kman_groups_extract up to
    each tile of cuts) -> (return code, n_kmers, rows or None)."""
    from kman_amd import _native as N

    L = N.lib()
    b = _Buffers(dev, c, mode, vb)
    try:
        nk, no = c_uint64(0), c_uint64(0)
        if cuts is None:
            r = L.kman_groups(*b.args(), *b.outs(nk, no))
        else:
            nt, tb = c_uint32(0), c_uint64(0)
            a = b.args()
            assert L.kman_groups_begin(a[0], *a[2:], byref(nt), byref(tb)) == N.KMAN_OK
            assert (nt.value, tb.value) == (c.plan.n_tiles0, c.plan.tile)
            for hi in cuts:
                assert L.kman_groups_extract(*a, hi) == N.KMAN_OK
            r = L.kman_groups_end(*a, *b.outs(nk, no))
        b.guards_intact()
        if r != N.KMAN_OK:
            return r, int(nk.value), None
        return r, int(nk.value), b.rows(int(no.value))
    finally:
        b.free()


def _general_keys(dev, monkeypatch, c, mode):
    """The keys of the general path (KMAN_NO_REGION=1: kman_extract_sorted +
    kman_finish) on the same text."""
    from kman_amd import engine

    monkeypatch.setenv("KMAN_NO_REGION", "1")
    try:
        p = engine.parse(dev, c.text)
        try:
            assert engine.groups(p, c.k, c.rc, mode, c.canonical) is None
            km = engine.extract_sorted(p, c.k, c.rc, want_pos=mode == "uniq", canonical=c.canonical)
            try:
                r = engine.rle_count(km, dev) if mode == "count" else engine.rle_uniq(km, dev)
            finally:
                km.free()
            try:
                return (engine.download_count if mode == "count" else engine.download_uniq)(dev, r)[0]
            finally:
                engine.free_result(r)
        finally:
            p.free()
    finally:
        monkeypatch.delenv("KMAN_NO_REGION")


def _assert_inside(dev, c, mode, vb, want, cuts=None):
    from kman_amd import _native as N

    r, nk, got = _call(dev, c, mode, vb, cuts)
    assert r == N.KMAN_OK, "a region filled to %d of %d left the region path (%d)" % (c.fill, c.cap, r)
    n, rows = want
    assert nk == n
    np.testing.assert_array_equal(got[0], rows[0])
    np.testing.assert_array_equal(got[1].astype(np.uint64), rows[1])
    return got


def _oracle_text(oracle_bin, tmp_path, c, mode):
    src, out = str(tmp_path / "in.fa"), str(tmp_path / "want.txt")
    with open(src, "wb") as fh:
        fh.write(c.text)
    subprocess.run([oracle_bin, mode, src, out, str(c.k)] + (["-r"] if c.rc else []), check=True)
    with open(out, "rb") as fh:
        return fh.read()


# Count items leave pass 1 as 4 bytes, and the narrow finish takes them, when
# the key bits below the region fit 32 (narrow_ok: rest <= 32).  At k = 21
# every plan here has rest = 33: 8-byte items with or without KMAN_WIDE_ITEMS.
# k = 20 (rest = 31) is the narrow path, and KMAN_WIDE_ITEMS=1 its wide twin.
NARROW_K = 20


# (edge, mode, k, rc, canonical, env, oval_bytes)
def _cases():
    out = []
    for e in R.EDGES:
        out += [(e, "count", 21, False, False, {}, 4), (e, "uniq", 21, False, False, {"KMAN_RG_CHECK": "0"}, 4),
                (e, "count", NARROW_K, False, False, {}, 4),
                (e, "count", NARROW_K, False, False, {"KMAN_WIDE_ITEMS": "1"}, 4), (e, "uniq", 21, False, False, {}, 4)]
    out += [
        ("c0_tile", "count", 9, False, False, {}, 4), ("fin_both", "count", 9, False, False, {}, 4),
        ("fin_both", "uniq", 13, False, False, {}, 4),
        ("c0_tile", "uniq", 21, True, False, {}, 4), ("c0_tile", "count", 21, True, False, {}, 4),
        ("c1_chain0", "count", 21, True, False, {}, 4), ("c1_chain0", "uniq", 21, True, False, {"KMAN_PASS_LINE1": "1"}, 4),
        ("fin_both", "count", 21, False, True, {}, 4),
        ("c0_seg3", "count", 21, False, False, {}, 8), ("fin_both", "uniq", 21, False, False, {}, 8),
        ("fin_m0", "count", NARROW_K, False, False, {}, 8),
    ]
    for e in ("c1_chain0", "c1_chain1"):  # the clamp min(fe, C1) of the one-line-per-digit pass
        out += [(e, "uniq", 21, False, False, {"KMAN_PASS_LINE1": "1", "KMAN_RG_CHECK": "0"}, 4),
                (e, "count", NARROW_K, False, False, {"KMAN_PASS_LINE1": "1"}, 4),
                (e, "count", NARROW_K, False, False, {"KMAN_PASS_LINE1": "1", "KMAN_WIDE_ITEMS": "1"}, 4)]
    return out


def _id(v):
    e, mode, k, rc, canonical, env, vb = v
    return "-".join([e, mode, "k%d" % k] + (["rc"] if rc else []) + (["canon"] if canonical else []) +
                    ["%s%s" % (n[5:].lower(), x) for n, x in sorted(env.items())] + ["v%d" % vb])


@pytest.mark.parametrize("delta", [-1, 0], ids=["cap-1", "cap"])
@pytest.mark.parametrize("case", _cases(), ids=_id)
def test_fill_up_to_the_capacity_stays_inside(dev, monkeypatch, case, delta):
    edge, mode, k, rc, canonical, env, vb = case
    c = R.build(edge, delta, k, rc, canonical)
    _assert_fills(c)
    _assert_item_width(c, mode, env)
    _set_env(monkeypatch, env)
    got = _assert_inside(dev, c, mode, vb, _want(edge, delta, k, rc, canonical, mode))
    np.testing.assert_array_equal(got[0], _general_keys(dev, monkeypatch, c, mode))


@pytest.mark.parametrize("case", _cases(), ids=_id)
def test_one_item_over_falls_back(dev, monkeypatch, oracle_bin, tmp_path, case):
    from kman_amd import _native as N
    from kman_amd import engine

    edge, mode, k, rc, canonical, env, vb = case
    over, full = R.build(edge, 1, k, rc, canonical), R.build(edge, 0, k, rc, canonical)
    _assert_fills(over)
    _assert_fills(full)
    assert over.fill == over.cap + 1 and full.fill == full.cap
    _assert_item_width(over, mode, env)
    _set_env(monkeypatch, env)
    r, _, rows = _call(dev, over, mode, vb)
    assert r == N.KMAN_EFALLBACK and rows is None, "%d items in a region of %d: %d" % (over.fill, over.cap, r)
    # the very next call on the context: the error word was cleared
    _assert_inside(dev, full, mode, vb, _want(edge, 0, k, rc, canonical, mode))
    if not env and not canonical and vb == 4:
        got = (engine.count_text if mode == "count" else engine.uniq_text)(over.text, k, rc=rc, dev=dev)
        assert got == _oracle_text(oracle_bin, tmp_path, over, mode)


@pytest.mark.parametrize("mode", ["count", "uniq"])
@pytest.mark.parametrize("delta", [-1, 0, 1], ids=["cap-1", "cap", "cap+1"])
def test_three_calls_cut_inside_the_target_segment(dev, monkeypatch, mode, delta):
    """kman_groups_begin / _extract / _end with every tile of the target
    segment in a launch of its own, so region (0, s)'s cursor is carried over
    launch boundaries and the last launch takes it to below, at or past C0:
    the verdicts and rows of the one-call form."""
    from kman_amd import _native as N

    c = R.build("c0_seg3", delta)
    _assert_fills(c)
    assert len(c.tiles) == 3 and c.tiles[-1] + 1 < c.plan.n_tiles0
    # (each of the three tiles brings a part of the fill, none of them all)
    _set_env(monkeypatch, {})
    cuts = [t + 1 for t in c.tiles]
    if delta <= 0:
        _assert_inside(dev, c, mode, 4, _want("c0_seg3", delta, 21, False, False, mode), cuts)
        return
    r, _, rows = _call(dev, c, mode, 4, cuts)
    assert r == N.KMAN_EFALLBACK and rows is None
    _assert_inside(dev, R.build("c0_seg3", 0), mode, 4, _want("c0_seg3", 0, 21, False, False, mode), cuts)


@pytest.mark.parametrize("cuts", [False, True], ids=["one-call", "three-calls"])
@pytest.mark.parametrize("mode", ["count", "uniq"])
def test_the_item_over_arrives_with_the_region_full(dev, monkeypatch, mode, cuts):
    """The segment's first two tiles bring exactly C0 items and its third only
    the item over: in the three-call form, a launch per tile in stream order,
    that tile finds the cursor at exactly C0 (the `at_base < C0 ? .. : 0` arm
    of qlim) and must store nothing.  Without the item the same layout is
    inside the path."""
    from kman_amd import _native as N

    _set_env(monkeypatch, {})
    full, over = R.build(R.LATE, 0), R.build(R.LATE, 1)
    for c in (full, over):
        _assert_fills(c)
        assert sum(c.tile_fills[:2]) == c.plan.C0 and min(c.tile_fills[:2]) > 0
    assert (full.tile_fills[2], over.tile_fills[2]) == (0, 1)
    hi = [t + 1 for t in over.tiles] if cuts else None
    r, _, rows = _call(dev, over, mode, 4, hi)
    assert r == N.KMAN_EFALLBACK and rows is None
    _assert_inside(dev, full, mode, 4, _want(R.LATE, 0, 21, False, False, mode), hi)


@pytest.mark.parametrize("mode", ["count", "uniq"])
def test_refusals_write_nothing(dev, monkeypatch, mode):
    """A work area one byte short is KMAN_ECAP, null codes KMAN_EINVAL:
    neither touches the work area, the outputs or the guards."""
    from kman_amd import _native as N

    _set_env(monkeypatch, {})
    c = R.build("c0_tile", 0)
    L = N.lib()
    b = _Buffers(dev, c, mode, 4, fill_all=True)
    try:
        nk, no = c_uint64(7), c_uint64(7)
        assert L.kman_groups(*b.args(work_bytes=b.wb - 1), *b.outs(nk, no)) == N.KMAN_ECAP
        assert (nk.value, no.value) == (0, 0)
        b.untouched()
        assert L.kman_groups(*b.args(codes=False), *b.outs(nk, no)) == N.KMAN_EINVAL
        b.untouched()
        # and the context still works
        assert L.kman_groups(*b.args(), *b.outs(nk, no)) == N.KMAN_OK
        b.guards_intact()
        n, rows = _want("c0_tile", 0, 21, False, False, mode)
        got = b.rows(int(no.value))
        assert nk.value == n
        np.testing.assert_array_equal(got[0], rows[0])
        np.testing.assert_array_equal(got[1].astype(np.uint64), rows[1])
    finally:
        b.free()
    assert os.environ.get("KMAN_NO_REGION") is None
