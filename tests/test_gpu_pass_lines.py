"""GPU parity of kman_groups' digit pass without a staged tile (region_pass.hip,
rg_pass<..., LN = true>): items ranked from registers into 256-byte
write-combining lines, whole lines stored in block-uniform rounds.

Every case goes through kman_groups itself and compares its rows bit-exactly
with np_oracle.  The lines body takes 8-byte items, so count runs set
KMAN_WIDE_ITEMS (count items of k <= 24 otherwise leave the pass as 4 bytes,
through the staged-tile body).  `line1` (KMAN_PASS_LINE1) gives every digit one
32-item line whatever the digit width, as the full-size pass (9 bits) has it:
a small input then completes many lines of one digit in one tile and takes one
placement round per line; without it a digit of a b-bit pass owns 2^(9 - b)
lines and a uniform tile takes one store phase."""

from __future__ import annotations

import functools
from ctypes import byref, c_uint64, c_void_p

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

# The repeat case: a 500-base unit, REPEAT_COPIES times in one record.  2000
# copies (1 Mbp) do not fit: no 17-bit prefix holds more than 2000 items, but
# at that size the plan makes 2^9 regions of 3456 items, a region holds 2000
# items per unit k-mer it gets, and the 500 k-mers put 5 into one of the 512
# (10 000 items).  Shortened until the fullest region stays inside its
# capacity: 750 of 768 items at 150 copies (200: 1000 of 832), which
# test_repeat_shape_stays_inside checks on the CPU.
REPEAT_UNIT, REPEAT_COPIES, REPEAT_SEED = 500, 150, 7


@pytest.fixture(scope="module")
def dev():
    from kman_amd import engine

    return engine.default_device()


@functools.lru_cache(maxsize=None)
def _text(name):
    import inputs

    if name == "syn12m":
        return inputs.syn_numpy(12_000_000, 21)
    if name == "syn100k":
        return inputs.syn_numpy(100_000, 5)
    if name == "syn3m":
        return inputs.syn_numpy(3_000_000, 6, record_len=1 << 20)
    if name == "repeat":
        rng = np.random.default_rng(REPEAT_SEED)
        unit = "".join(rng.choice(list("ACGT"), REPEAT_UNIT))
        return b">rep\n" + (unit * REPEAT_COPIES).encode() + b"\n"
    if name == "overflow":  # (test_gpu_region.test_groups_overflow_falls_back's input)
        return b">a\n" + b"A" * 300_000 + b"\n>b\n" + b"ACGT" * 1000 + b"\n"
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def _sorted(text, k, rc):
    """The stream's (key, pos) stably sorted: once per (input, k, rc), shared
    by the count and uniq cases (read-only)."""
    import np_oracle

    keys, pos = np_oracle.stream_kmers(np_oracle.parse_fasta(text), k, rc=rc)
    sk, sp = np_oracle.stable_sort(keys, pos)
    sk.setflags(write=False)
    sp.setflags(write=False)
    return sk, sp


def _oracle(text, k, rc, mode):
    import np_oracle

    sk, sp = _sorted(text, k, rc)
    return np_oracle.rle_count(sk) if mode == "count" else np_oracle.rle_uniq(sk, sp)


def _plan(W):
    """region_groups.hip's make_plan for W k-mer slots: pass-1 bits and sub-region
    capacity."""
    b2 = 1
    while b2 < 9 and (W >> (8 + b2)) > 6144:
        b2 += 1
    e1 = W >> (8 + b2)
    return b2, min(8704, -(-(e1 + e1 // 2 + 512) // 64) * 64)


def _kman_groups(dev, text, k, rc, mode):
    """kman_groups by ctypes: (return code, rows or None)."""
    from kman_amd import _native as N
    from kman_amd import engine

    L = N.lib()
    p = engine.parse(dev, text)
    bufs = []
    try:
        m = N.KMAN_FINISH_UNIQ if mode == "uniq" else N.KMAN_FINISH_COUNT
        flags = engine.flags_for(rc, mode == "uniq")
        wb = c_uint64(0)
        assert L.kman_groups_plan(p.n_bases, k, flags, m, byref(wb)) == N.KMAN_OK
        cap = p.n_bases * (2 if rc else 1)
        work, okeys, ovals = dev.alloc(int(wb.value)), dev.alloc(8 * cap), dev.alloc(4 * cap)
        bufs += [work, okeys, ovals]
        assert work.ptr % 256 == 0  # (the lines body needs it; otherwise the staged tile runs)
        nk, no = c_uint64(0), c_uint64(0)
        r = L.kman_groups(dev.ctx, c_void_p(p.codes.ptr), p.n_bases, k, flags, m, c_void_p(work.ptr), wb.value,
                          c_void_p(okeys.ptr), c_void_p(ovals.ptr), 4, byref(nk), byref(no))
        if r != N.KMAN_OK:
            return r, None
        n = int(no.value)
        return r, (dev.download(okeys, n, np.uint64), dev.download(ovals, n, np.uint32))
    finally:
        for b in bufs:
            b.free()
        p.free()


def _check(dev, monkeypatch, text, k, rc, mode, line1):
    from kman_amd import _native as N

    monkeypatch.setenv("KMAN_WIDE_ITEMS", "1")
    if line1:
        monkeypatch.setenv("KMAN_PASS_LINE1", "1")
    else:
        monkeypatch.delenv("KMAN_PASS_LINE1", raising=False)
    r, got = _kman_groups(dev, text, k, rc, mode)
    assert r == N.KMAN_OK, "an input inside the region path fell back"
    want = _oracle(text, k, rc, mode)
    np.testing.assert_array_equal(got[0], want[0])
    np.testing.assert_array_equal(got[1].astype(np.uint64), want[1])


@pytest.mark.parametrize("line1", [False, True])
@pytest.mark.parametrize("rc", [False, True])
@pytest.mark.parametrize("mode", ["uniq", "count"])
def test_several_tiles_per_chain(dev, monkeypatch, mode, rc, line1):
    """12 Mbp: ~47 K items per bucket, ~3 tiles in each of a bucket's two
    chains -- lines carried from tile to tile and flushed at the chain end."""
    _check(dev, monkeypatch, _text("syn12m"), 21, rc, mode, line1)


@pytest.mark.parametrize("line1", [False, True])
@pytest.mark.parametrize("mode", ["uniq", "count"])
@pytest.mark.parametrize("name", ["syn100k", "syn3m"])
def test_one_ragged_tile_per_chain(dev, monkeypatch, name, mode, line1):
    """One tile or less per chain, the last one ragged: most digits end with
    a partial line only (and the second chain of a bucket is empty)."""
    _check(dev, monkeypatch, _text(name), 21, False, mode, line1)


def _repeat_fill():
    """(fullest region, capacity) of the repeat case, from the oracle's keys."""
    sk, _ = _sorted(_text("repeat"), 21, False)
    b2, c1 = _plan(REPEAT_UNIT * REPEAT_COPIES)
    fill = np.bincount((sk >> np.uint64(42 - 8 - b2)).astype(np.int64), minlength=1 << (8 + b2))
    return int(fill.max()), c1


def test_repeat_shape_stays_inside():
    """(CPU) no region of the repeat case holds more than its capacity -- all
    of a region's items may come through one chain, so its sub-region's."""
    most, c1 = _repeat_fill()
    assert REPEAT_COPIES * 5 == most <= c1


@pytest.mark.parametrize("line1", [False, True])
@pytest.mark.parametrize("mode", ["uniq", "count"])
def test_many_lines_of_one_digit(dev, monkeypatch, mode, line1):
    """Every key REPEAT_COPIES times: a bucket's tile holds a handful of
    digits with hundreds of items each, so (line1) a digit completes ten and
    more lines in one tile; no region overflows."""
    _check(dev, monkeypatch, _text("repeat"), 21, False, mode, line1)


@pytest.mark.parametrize("line1", [False, True])
@pytest.mark.parametrize("mode", ["uniq", "count"])
def test_overflow_still_falls_back(dev, monkeypatch, mode, line1):
    """One k-mer 300 K times: its region overflows, nothing is written past
    a capacity, kman_groups itself says KMAN_EFALLBACK, and the engine's rows
    (through the general path) are the oracle's."""
    from kman_amd import _native as N
    from kman_amd import engine

    monkeypatch.setenv("KMAN_WIDE_ITEMS", "1")
    if line1:
        monkeypatch.setenv("KMAN_PASS_LINE1", "1")
    text = _text("overflow")
    r, got = _kman_groups(dev, text, 21, False, mode)
    assert r == N.KMAN_EFALLBACK and got is None
    out = (engine.count_text if mode == "count" else engine.uniq_text)(text, 21, dev=dev)
    want = _oracle(text, 21, False, mode)
    if mode == "count":
        lines = out.decode().splitlines()
        assert len(lines) == len(want[0])
        assert [int(x.split("\t")[1]) for x in lines] == want[1].tolist()
    else:
        assert out.count(b">") == len(want[0])
    # the context is clean again: the next call inside the path is exact
    _check(dev, monkeypatch, _text("syn100k"), 21, False, mode, line1)


@pytest.mark.parametrize("rc", [False, True])
@pytest.mark.parametrize("mode", ["uniq", "count"])
def test_region_counts_off_the_line(dev, golden_inputs, monkeypatch, mode, rc):
    """A messy golden file at k = 13: record and segment boundaries leave
    region counts that are no multiples of 32."""
    from kman_amd.engine import read_input

    text = read_input(golden_inputs["messy1"])
    import np_oracle

    sk, _ = _sorted(text, 13, rc)
    b2, _c1 = _plan(sum(len(s) for _, s in np_oracle.parse_fasta(text)) * (2 if rc else 1))
    fill = np.bincount((sk >> np.uint64(26 - 8 - b2)).astype(np.int64), minlength=1 << (8 + b2))
    assert (fill % 32 != 0).any()
    for line1 in (False, True):
        _check(dev, monkeypatch, text, 13, rc, mode, line1)
