"""`kmer screen --median` without a GPU: the plain-Python statement
(tests/median_cases.py) pinned to hand-worked cases, the host formatter
kman_format_screen_median, engine.screen_keep's median keywords, the CLI's
refusals (raised before any device work or output file), the plan call and
the ABI's constants."""

from __future__ import annotations

import ctypes
import os
import re
from ctypes import byref, c_size_t, c_uint64, c_void_p

import numpy as np
import pytest
from click.testing import CliRunner

import median_cases as mc
import screen_cases as sc

NONE = mc.NONE


def test_quantile_rule_on_hand_worked_cases():
    assert mc.quantile([]) == 0                       # w = 0
    assert mc.quantile([NONE, NONE]) == 0
    assert mc.quantile([7]) == 7                      # w = 1
    assert mc.quantile([NONE, 7, NONE], 0, 1) == mc.quantile([NONE, 7, NONE], 1, 1) == 7
    assert mc.quantile([9, 3]) == 3                   # w = 2: the lower median
    assert mc.quantile([9, 3], 1, 1) == 9 and mc.quantile([9, 3], 0, 1) == 3
    assert mc.quantile([5, 1, 9]) == 5                # w = 3
    assert mc.quantile([4, NONE, 1, 3, 2]) == 2       # w = 4 (even): index (4 - 1) // 2 = 1
    assert mc.quantile([4, 1, 3, 2], 3, 4) == 3       # index 3 * 3 // 4 = 2
    assert mc.quantile([4, 1, 3, 2], 1, 4) == 1       # index 3 * 1 // 4 = 0
    assert mc.quantile([0, mc.SAT, 0, mc.SAT, mc.SAT]) == mc.SAT
    vals = list(range(100, 0, -1))
    assert mc.quantile(vals, 99, 100) == 99 and mc.quantile(vals, 65535, 65535) == 100
    assert mc.quantile(vals, 0, 1) == min(vals) and mc.quantile(vals, 1, 1) == max(vals)
    # records: the last one runs to n_bases, equal entries are empty, entries are clamped
    words = [5, NONE, 1, 2, 3, NONE, NONE, 8]
    assert mc.record_quantiles(words, [0, 2, 2, 5, 99], 8) == [5, 0, 2, 8, 0]
    assert mc.record_quantiles(words, [1, 5], 8, 1, 1) == [3, 8]  # base 0 belongs to nobody


def test_window_words_on_a_hand_written_example():
    """k = 3, the table of test_screen_cpu's example."""
    table = {"ACG": 2, "CGT": 1, "GTA": 1, "TAC": 1, "TTT": 1 << 40}
    reads = [("all", "ACGTA"), ("short", "AC"), ("empty", ""), ("masked", "ACGNTTTn"), ("lower", "ttta")]
    want = [2, 1, 1, NONE, NONE,  NONE, NONE,  2, NONE, NONE, NONE, mc.SAT, NONE, NONE, NONE,  mc.SAT, 0, NONE, NONE]
    assert mc.window_words(reads, 3, table) == want
    assert mc.medians(reads, 3, table) == [1, 0, 0, 2, 0]
    assert mc.medians(reads, 3, table, num=1, den=1) == [2, 0, 0, mc.SAT, mc.SAT]
    ctable = {"ACG": 3, "GTA": 2, "AAA": 1}
    assert mc.window_words(reads[:1], 3, ctable, True) == [3, 3, 2, NONE, NONE]
    st = sc.stats(reads, 3, table)
    assert [int(x) for x in st[:, 0]] == [sum(1 for x in mc.window_words([r], 3, table) if x != NONE) for r in reads]
    small = {w: 1 for w in table}
    assert mc.property_holds(sc.stats(reads, 3, small), mc.medians(reads, 3, small))
    assert not mc.property_holds([(3, 3, 3)], [0])


# ------------------------------------------------------------ host formatter


def _format(st, med, names, keep=None, cap=None, threads=3):
    from kman_amd import _native as N

    L = ctypes.CDLL(N.LIB_PATH)  # (the formatter is host code: no device is asked for)
    fn = L.kman_format_screen_median
    fn.restype, fn.argtypes = N.SIGNATURES["kman_format_screen_median"]
    st = np.asarray(st, dtype=np.uint64).reshape(-1, 3)
    n = st.shape[0]
    planes = np.ascontiguousarray(st.T)
    med = np.ascontiguousarray(med, dtype=np.uint32)
    blob = b"".join(names)
    off = np.zeros(n + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(x) for x in names])
    kp = None
    if keep is not None:
        keep = np.asarray(keep, dtype=np.uint8)
        kp = keep.ctypes.data_as(c_void_p)
    used = c_size_t(0)
    buf = ctypes.create_string_buffer(max(1, cap)) if cap is not None else None
    rc = fn(planes.ctypes.data_as(c_void_p), med.ctypes.data_as(c_void_p), n, kp, blob, off.ctypes.data_as(c_void_p),
            buf, cap or 0, byref(used), threads)
    return rc, used.value, (buf.raw[:used.value] if buf is not None and rc == 0 else None)


def test_format_screen_median():
    from kman_amd import _native as N

    big = (1 << 64) - 1
    st = [(136, 0, 0), (0, 0, 0), (5, 5, (1 << 32) + 7), (1 << 33, (1 << 32) + 1, big), (10, 3, 999), (7, 7, 7)]
    med = [0, 0, mc.SAT, 12, 4294967295, 1]
    names = [b"read1", b"", b"with\ttab", b"r/1", b"x" * 300, b"last"]
    recs = [(n.decode(), "") for n in names]
    want = mc.lines(recs, st, med)
    assert b"with\ttab\t5\t5\t4294967303\t4294967294\n" in want and b"\n\t0\t0\t0\t0\n" in want
    rc, used, _ = _format(st, med, names)  # sizing call: no buffer
    assert (rc, used) == (N.KMAN_ECAP, len(want))
    rc, used, text = _format(st, med, names, cap=len(want))
    assert (rc, used, text) == (N.KMAN_OK, len(want), want)
    rc, used, _ = _format(st, med, names, cap=len(want) - 1)  # one byte short: refused, the size reported
    assert (rc, used) == (N.KMAN_ECAP, len(want))
    for keep in ([1, 0, 1, 0, 0, 1], [0] * 6, [1] * 6, [0, 1, 0, 0, 0, 0], [0, 2, 0, 0, 255, 0]):
        w = mc.lines(recs, st, med, keep)
        rc, used, text = _format(st, med, names, keep, cap=len(w) + 16)
        assert (rc, used, text) == (N.KMAN_OK, len(w), w), keep
    assert _format([], [], [], cap=8) == (N.KMAN_OK, 0, b"")
    rng = np.random.default_rng(5)
    n = 20_000
    st = rng.integers(0, 1 << 40, (n, 3), dtype=np.uint64)
    med = rng.integers(0, 1 << 32, n, dtype=np.uint64)
    names = [b"n%d" % i for i in range(n)]
    keep = rng.integers(0, 2, n).astype(np.uint8)
    w = mc.lines([(x.decode(), "") for x in names], st, med, keep)
    for threads in (1, 4):
        rc, used, text = _format(st, med, names, keep, cap=len(w), threads=threads)
        assert (rc, used) == (N.KMAN_OK, len(w)) and text == w


# --------------------------------------------------------------- screen_keep


def test_screen_keep_median_keywords():
    from kman_amd import engine

    rng = np.random.default_rng(11)
    n = 500
    w = rng.integers(0, 140, n)
    h = (w * rng.random(n)).astype(np.int64)
    st = np.stack([w, h, h * 3], axis=1).astype(np.uint64)
    med = rng.integers(0, 9, n).astype(np.uint32)
    med[:5] = [0, mc.SAT, 3, 4, 5]
    for mh, mf, inv in ((0, 0.0, False), (3, 0.0, False), (0, 0.5, True), (2, 0.25, False), (0, 0.0, True)):
        today = engine.screen_keep(st, mh, mf, inv)
        assert today.tolist() == [int(x) for x in sc.keep(st, mh, mf, inv)]
        # the defaults, and a median without bounds, reproduce today's mask
        assert engine.screen_keep(st, mh, mf, inv, median=None, min_median=None, max_median=None).tobytes() == \
            today.tobytes()
        assert engine.screen_keep(st, mh, mf, inv, median=med).tobytes() == today.tobytes()
        for lo, hi in ((3, None), (None, 4), (3, 5), (0, 0), (5, 3), (mc.SAT, None), (None, 0), (1 << 33, None)):
            got = engine.screen_keep(st, mh, mf, inv, median=med, min_median=lo, max_median=hi)
            want = mc.keep(st, med, mh, mf, inv, lo, hi)
            assert got.dtype == np.uint8 and got.tolist() == [int(x) for x in want], (mh, mf, inv, lo, hi)
    assert 0 < engine.screen_keep(st, median=med, min_median=3, max_median=5).sum() < n
    with pytest.raises(TypeError):
        engine.screen_keep(st, 0, 0.0, False, med)  # keyword-only
    with pytest.raises(AssertionError):
        engine.screen_keep(st, min_median=1)  # a bound without the array


# ----------------------------------------------------------------------- CLI


@pytest.fixture()
def inputs(tmp_path):
    fa = tmp_path / "reads.fa"
    fa.write_bytes(b">r\nACGTACGTTGCAACGT\n")
    fb = tmp_path / "genome.fa"
    fb.write_bytes(b">s\nTTGCAACGTACG\n")
    return fa, fb


def test_help_shows_the_median_options():
    from kman_amd.scripts.kmer import main

    text = CliRunner().invoke(main, ["screen", "--help"]).output
    for opt in ("--median", "--min-median", "--max-median", "MEDIAN"):
        assert opt in text, opt


REFUSED = {
    "min_above_max": (["5", "--min-median", "6", "--max-median", "5"], "--min-median 6 is greater than --max-median 5"),
    "min_negative": (["5", "--min-median=-1"], "--min-median"),
    "max_negative": (["5", "--median", "--max-median=-3"], "--max-median"),
}


@pytest.mark.parametrize("case", sorted(REFUSED))
def test_refused_before_any_device_work_or_output(case, inputs, tmp_path, monkeypatch):
    from kman_amd import _native, engine
    from kman_amd.scripts.kmer import main

    def no_device(*a, **kw):
        raise RuntimeError("device work before the options were checked")

    monkeypatch.setattr(engine, "default_device", no_device)
    monkeypatch.setattr(engine, "Device", no_device)
    monkeypatch.setattr(_native, "lib", no_device)
    argv, msg = REFUSED[case]
    out = tmp_path / "out.tsv"
    r = CliRunner().invoke(main, ["screen", str(inputs[0]), str(inputs[1]), str(out)] + argv)
    assert isinstance(r.exception, AssertionError), (r.exception, r.output)
    assert msg in str(r.exception)
    assert not out.exists()


def test_usage_errors(inputs, tmp_path):
    from kman_amd.scripts.kmer import main

    out = tmp_path / "out.tsv"
    for argv in (["5", "--min-median", "x"], ["5", "--max-median", "1.5"], ["5", "--median", "3"]):
        r = CliRunner().invoke(main, ["screen", str(inputs[0]), str(inputs[1]), str(out)] + argv)
        assert r.exit_code == 2 and not out.exists(), argv


@pytest.mark.parametrize("argv", [["--median"], ["--min-median", "2"], ["--max-median", "2"]])
def test_each_option_asks_for_the_median(argv, inputs, tmp_path, monkeypatch):
    """Either bound alone implies --median: the command reaches screen_median."""
    from kman_amd import engine
    from kman_amd.scripts import kmer

    class Reached(Exception):
        pass

    class _Table:
        pass

    class _Parsed:
        def free(self):
            pass

    def reached(*a, **kw):
        raise Reached()

    def not_wanted(*a, **kw):
        raise RuntimeError("engine.screen without the median")

    for v in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "KMAN_DIST"):
        monkeypatch.delenv(v, raising=False)
    monkeypatch.setattr(engine, "default_device", lambda *a, **kw: None)
    monkeypatch.setattr(engine, "parse_file", lambda *a, **kw: _Parsed())
    monkeypatch.setattr(engine, "check_empty_names", lambda *a, **kw: None)
    monkeypatch.setattr(engine, "join_groups", lambda *a, **kw: _Table())
    monkeypatch.setattr(engine, "free_result", lambda *a, **kw: None)
    monkeypatch.setattr(engine, "screen_median", reached)
    monkeypatch.setattr(engine, "screen", not_wanted)
    out = tmp_path / "out.tsv"
    r = CliRunner().invoke(kmer.main, ["screen", str(inputs[0]), str(inputs[1]), str(out), "5"] + argv)
    assert isinstance(r.exception, Reached), (r.exception, r.output)
    assert not out.exists()


# ------------------------------------------------------------ plan, constants


def test_plan_call():
    from kman_amd import _native as N

    L = ctypes.CDLL(N.LIB_PATH)  # (host only: no device is asked for)
    fn = L.kman_record_quantile_plan
    fn.restype, fn.argtypes = N.SIGNATURES["kman_record_quantile_plan"]

    def plan(nl, nv):
        out = c_uint64(123)
        rc = fn(nl, nv, byref(out))
        return rc, out.value

    rc, base = plan(0, 0)
    assert rc == N.KMAN_OK and 0 < base <= 4096  # (the size a call with only short records accepts: GPU test)
    C = N.KMAN_QUANTILE_REC_CAP
    rc, one = plan(1, C + 1)
    assert rc == N.KMAN_OK and one >= base + 16 * (C + 1)  # keys and the sort's second buffer
    assert plan(3, 10 * C)[1] > plan(2, 10 * C)[1] > plan(2, 9 * C)[1]
    assert fn(0, 0, None) == N.KMAN_EINVAL
    assert plan(1 << 33, 1 << 40)[0] == N.KMAN_EINVAL


def test_quantile_plan_of_a_record_table():
    from kman_amd import _native as N
    from kman_amd import engine

    C = N.KMAN_QUANTILE_REC_CAP
    lens = [0, 1, C, C + 1, 5, 3 * C, 0, C + 7]
    rs = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.uint64)
    assert engine.quantile_plan(rs, sum(lens)) == (3, C + 1 + 3 * C + C + 7)
    assert engine.quantile_plan(rs[:3], 1 + C) == (0, 0)  # (the third record: bases [1, 1 + C), the last short length)
    assert engine.quantile_plan(rs[:3], 2 + C) == (1, C + 1)
    assert engine.quantile_plan(rs, sum(lens) - 7) == (2, C + 1 + 3 * C)  # the last record is cut at n_bases
    assert engine.quantile_plan(np.zeros(0, np.uint64), 50) == (0, 0)


def test_header_signatures_and_constants_agree():
    from kman_amd import _native as N

    with open(os.path.join(os.path.dirname(N.HERE), "include", "kman.h")) as fh:
        text = fh.read()
    for name in ("KMAN_QUANTILE_TILE", "KMAN_QUANTILE_REC_CAP", "KMAN_QUANTILE_SLICE"):
        m = re.search(r"#define\s+%s\s+(\d+)\s" % name, text)
        assert m and int(m.group(1)) == getattr(N, name), name
    m = re.search(r"#define\s+KMAN_WC_NONE\s+0x([0-9A-Fa-f]+)u\s", text)
    assert m and int(m.group(1), 16) == N.KMAN_WC_NONE == mc.NONE == 0xFFFFFFFF
    assert N.KMAN_QUANTILE_TILE % 4 == 0 and N.KMAN_QUANTILE_REC_CAP >= 1024  # (a 150- or 1000-base read is short)
    syms = N.header_symbols()
    for name, nargs in (("kman_window_counts", 12), ("kman_record_quantile_plan", 3), ("kman_record_quantile", 10),
                        ("kman_format_screen_median", 10), ("kman_format_screen", 9)):
        assert name in syms and name in N.SIGNATURES, name
        assert len(N.SIGNATURES[name][1]) == nargs, name
        decl = re.search(r"\bint %s\(([^;]*)\);" % name, text)
        assert decl and len(decl.group(1).split(",")) == nargs, name
    assert sorted(N.SIGNATURES) == syms
    assert re.search(r"#define\s+KMAN_ABI_VERSION\s+1\s", text)
    with open(os.path.join(N.HERE, "csrc", "quantile.hip")) as fh:
        src = fh.read()
    for line in ("static_assert(QC == KMAN_QUANTILE_TILE", "static_assert(QCAP == KMAN_QUANTILE_REC_CAP",
                 "static_assert(QSLICE == KMAN_QUANTILE_SLICE", "static_assert(WTILE == KMAN_SCREEN_TILE"):
        assert line in src, line
    # one lookup: both kernels call the shared device function
    with open(os.path.join(N.HERE, "csrc", "screen.hip")) as fh:
        scr = fh.read()
    assert "table_lookup<" in src and "table_lookup<" in scr and '#include "screen_lookup.h"' in scr
    with open(os.path.join(N.HERE, "csrc", "Makefile")) as fh:
        assert "quantile.hip" in fh.read()
