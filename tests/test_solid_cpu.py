"""`kmer screen --solid` without a GPU: the plain-Python statement
(tests/solid_cases.py) pinned to hand-worked cases, engine.solid_spans,
engine.screen_keep's span keywords, the host formatters
kman_format_screen_solid and kman_format_bed, the CLI's refusals (raised
before any device work or output file), the plan call and the ABI's
constants."""

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
import solid_cases as so

NONE = so.NONE


def test_run_rule_on_hand_worked_cases():
    assert so.longest_run([], 1) == (0, 0)
    assert so.longest_run([NONE, NONE], 1) == (0, 0)
    assert so.longest_run([0, 0, 0], 1) == (0, 0)              # a count of 0 is never solid
    assert so.longest_run([5], 5) == (0, 1) and so.longest_run([4], 5) == (0, 0)
    assert so.longest_run([1, 1, NONE, 1, 1], 1) == (0, 2)     # a tie: the leftmost
    assert so.longest_run([1, NONE, 1, 1, 0, 1, 1, 1], 1) == (5, 3)  # a longer one later wins
    assert so.longest_run([3, 2, 3, 3, 2, 3], 3) == (2, 2)
    assert so.longest_run([NONE - 1, NONE, NONE - 2], NONE - 1) == (0, 1)
    words = [2, 2, 2, 2, NONE, 2, 2, 2]
    # a run is cut at a record's end although the neighbour's words are solid
    assert so.record_runs(words, [0, 2, 2, 5, 99], 8, 2) == [(0, 2), (0, 0), (0, 2), (0, 3), (0, 0)]
    assert so.record_runs(words, [1, 5], 8, 1) == [(0, 3), (0, 3)]   # base 0 belongs to nobody
    assert so.record_runs(words, [0], 8, 3) == [(0, 0)]
    assert so.spans([(0, 0), (4, 1), (2, 10)], 21) == [(0, 0), (4, 25), (2, 32)]


def test_runs_of_a_hand_written_example():
    """k = 3: the words of test_median_cpu's example; an N and a record's end stop a stretch."""
    table = {"ACG": 2, "CGT": 1, "GTA": 1, "TAC": 1, "TTT": 1 << 40}
    reads = [("all", "ACGTA"), ("short", "AC"), ("empty", ""), ("masked", "ACGNTTTn"), ("lower", "ttta")]
    assert so.runs_of(reads, 3, table, 1) == [(0, 3), (0, 0), (0, 0), (0, 1), (0, 1)]
    assert so.runs_of(reads, 3, table, 2) == [(0, 1), (0, 0), (0, 0), (0, 1), (0, 1)]
    assert so.runs_of(reads, 3, table, 3) == [(0, 0), (0, 0), (0, 0), (4, 1), (0, 1)]
    sp = so.spans(so.runs_of(reads, 3, table, 3), 3)
    assert sp == [(0, 0), (0, 0), (0, 0), (4, 7), (0, 3)]
    assert so.cut(reads, sp) == ["TTT", "ttt"]   # the bases of the solid windows, N excluded
    # an error in mid-read: the k windows over it are weak, the longer side is the stretch
    good = "ACGTTGCATGCCAGTAAGCT"
    t5 = sc.table_of([("g", good)] * 3, 5)
    bad = good[:12] + "T" + good[13:]
    assert so.runs_of([("bad", bad)], 5, t5, 3) == [(0, 8)]
    assert so.cut([("bad", bad)], so.spans([(0, 8)], 5)) == [good[:12]]


def test_solid_spans():
    from kman_amd import engine

    runs = np.asarray([(0, 0), (4, 1), (2, 10), (7, 0), (0, 130), ((1 << 33) + 5, (1 << 32) + 1)], dtype=np.uint64)
    for k in (2, 21, 32):
        start, end = engine.solid_spans(runs, k)
        assert start.dtype == end.dtype == np.uint64 and start.shape == end.shape == (len(runs),)
        assert list(zip(start.tolist(), end.tolist())) == so.spans(runs.tolist(), k)
    start, end = engine.solid_spans(np.zeros((0, 2), np.uint64), 5)
    assert start.shape == end.shape == (0,)
    assert engine.solid_spans(runs, 21)[1][3] == 0   # a start without a length: no span


def test_screen_keep_span_keywords():
    from kman_amd import engine

    rng = np.random.default_rng(12)
    n = 400
    w = rng.integers(0, 140, n)
    h = (w * rng.random(n)).astype(np.int64)
    st = np.stack([w, h, h * 3], axis=1).astype(np.uint64)
    med = rng.integers(0, 9, n).astype(np.uint32)
    runs = np.stack([rng.integers(0, 50, n), rng.integers(0, 100, n)], axis=1).astype(np.uint64)
    runs[:4] = [(0, 0), (0, 1), (3, 0), (0, 130)]
    span = engine.solid_spans(runs, 21)
    sp = so.spans(runs.tolist(), 21)
    for mh, mf, inv in ((0, 0.0, False), (3, 0.0, False), (0, 0.5, True), (0, 0.0, True)):
        today = engine.screen_keep(st, mh, mf, inv)
        # the defaults, and a span without a bound, reproduce today's mask
        assert engine.screen_keep(st, mh, mf, inv, span=None, min_solid_len=None).tobytes() == today.tobytes()
        assert engine.screen_keep(st, mh, mf, inv, span=span).tobytes() == today.tobytes()
        assert today.tolist() == [int(x) for x in so.keep(st, sp, mh, mf, inv)]
        for nmin in (0, 1, 21, 22, 60, 150, 1 << 40):
            got = engine.screen_keep(st, mh, mf, inv, span=span, min_solid_len=nmin)
            assert got.dtype == np.uint8
            assert got.tolist() == [int(x) for x in so.keep(st, sp, mh, mf, inv, nmin)], (mh, mf, inv, nmin)
        got = engine.screen_keep(st, mh, mf, inv, median=med, min_median=2, max_median=6, span=span, min_solid_len=40)
        assert got.tolist() == [int(x) for x in so.keep(st, sp, mh, mf, inv, 40, med, 2, 6)]
    assert 0 < engine.screen_keep(st, span=span, min_solid_len=60).sum() < n
    assert engine.screen_keep(st, span=span, min_solid_len=0).all()          # 0 keeps a record without a span
    assert not engine.screen_keep(st, span=span, min_solid_len=1)[0]         # (0, 0): no base
    with pytest.raises(TypeError):
        engine.screen_keep(st, 0, 0.0, False, None, None, None, span)  # keyword-only
    with pytest.raises(AssertionError):
        engine.screen_keep(st, min_solid_len=1)  # a bound without the arrays
    with pytest.raises(AssertionError):
        engine.screen_keep(st, span=(span[0][:-1], span[1][:-1]), min_solid_len=1)


# ------------------------------------------------------------ host formatters


def _names(names):
    blob = b"".join(names)
    off = np.zeros(len(names) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(x) for x in names])
    return blob, off


def _call(name, head, names, keep, cap, threads):
    from kman_amd import _native as N

    L = ctypes.CDLL(N.LIB_PATH)  # (the formatters are host code: no device is asked for)
    fn = getattr(L, name)
    fn.restype, fn.argtypes = N.SIGNATURES[name]
    blob, off = _names(names)
    kp = None
    if keep is not None:
        keep = np.asarray(keep, dtype=np.uint8)
        kp = keep.ctypes.data_as(c_void_p)
    used = c_size_t(0)
    buf = ctypes.create_string_buffer(max(1, cap)) if cap is not None else None
    rc = fn(*head, len(names), kp, blob, off.ctypes.data_as(c_void_p), buf, cap or 0, byref(used), threads)
    return rc, used.value, (buf.raw[:used.value] if buf is not None and rc == 0 else None)


def _format_solid(st, med, span, names, keep=None, cap=None, threads=3):
    st = np.asarray(st, dtype=np.uint64).reshape(-1, 3)
    planes = np.ascontiguousarray(st.T)
    m = np.ascontiguousarray(med, dtype=np.uint32) if med is not None else None
    start = np.ascontiguousarray([a for a, _ in span], dtype=np.uint64)
    end = np.ascontiguousarray([b for _, b in span], dtype=np.uint64)
    head = (planes.ctypes.data_as(c_void_p), m.ctypes.data_as(c_void_p) if m is not None else None,
            start.ctypes.data_as(c_void_p), end.ctypes.data_as(c_void_p))
    return _call("kman_format_screen_solid", head, names, keep, cap, threads)


def _format_bed(span, names, keep=None, cap=None, threads=3):
    start = np.ascontiguousarray([a for a, _ in span], dtype=np.uint64)
    end = np.ascontiguousarray([b for _, b in span], dtype=np.uint64)
    return _call("kman_format_bed", (start.ctypes.data_as(c_void_p), end.ctypes.data_as(c_void_p)), names, keep, cap,
                 threads)


BIG = (1 << 64) - 1
ST = [(136, 0, 0), (0, 0, 0), (5, 5, (1 << 32) + 7), (1 << 33, (1 << 32) + 1, BIG), (10, 3, 999), (7, 7, 7)]
MED = [0, 0, mc.SAT, 12, 4294967295, 1]
SPAN = [(0, 0), (0, 0), (0, 25), (1 << 33, (1 << 34) + 20), (4, 5), (129, 150)]
NAMES = [b"read1", b"", b"with\ttab", b"r/1", b"x" * 300, b"last"]
KEEPS = ([1, 0, 1, 0, 0, 1], [0] * 6, [1] * 6, [0, 1, 0, 0, 0, 0], [0, 2, 0, 0, 255, 0])


@pytest.mark.parametrize("with_median", [False, True])
def test_format_screen_solid(with_median):
    from kman_amd import _native as N

    med = MED if with_median else None
    recs = [(n.decode(), "") for n in NAMES]
    want = so.lines(recs, ST, SPAN, med)
    if with_median:
        assert b"with\ttab\t5\t5\t4294967303\t4294967294\t0\t25\n" in want and b"\n\t0\t0\t0\t0\t0\t0\n" in want
    else:
        assert b"with\ttab\t5\t5\t4294967303\t0\t25\n" in want and b"\n\t0\t0\t0\t0\t0\n" in want
        assert b"last\t7\t7\t7\t129\t150\n" in want
    rc, used, _ = _format_solid(ST, med, SPAN, NAMES)  # sizing call: no buffer
    assert (rc, used) == (N.KMAN_ECAP, len(want))
    rc, used, text = _format_solid(ST, med, SPAN, NAMES, cap=len(want))
    assert (rc, used, text) == (N.KMAN_OK, len(want), want)
    rc, used, _ = _format_solid(ST, med, SPAN, NAMES, cap=len(want) - 1)  # one byte short: refused, the size reported
    assert (rc, used) == (N.KMAN_ECAP, len(want))
    for keep in KEEPS:
        w = so.lines(recs, ST, SPAN, med, keep)
        rc, used, text = _format_solid(ST, med, SPAN, NAMES, keep, cap=len(w) + 16)
        assert (rc, used, text) == (N.KMAN_OK, len(w), w), keep
    assert _format_solid([], [] if with_median else None, [], [], cap=8) == (N.KMAN_OK, 0, b"")
    rng = np.random.default_rng(6)
    n = 20_000
    st = rng.integers(0, 1 << 40, (n, 3), dtype=np.uint64)
    m = rng.integers(0, 1 << 32, n, dtype=np.uint64) if with_median else None
    a = rng.integers(0, 1 << 20, n)
    span = list(zip(a.tolist(), (a + rng.integers(0, 300, n)).tolist()))
    names = [b"n%d" % i for i in range(n)]
    keep = rng.integers(0, 2, n).astype(np.uint8)
    w = so.lines([(x.decode(), "") for x in names], st, span, m, keep)
    for threads in (1, 4):
        rc, used, text = _format_solid(st, m, span, names, keep, cap=len(w), threads=threads)
        assert (rc, used) == (N.KMAN_OK, len(w)) and text == w


def test_format_bed():
    from kman_amd import _native as N

    recs = [(n.decode(), "") for n in NAMES]
    want = so.bed(recs, SPAN)
    assert want == b"with\ttab\t0\t25\nr/1\t8589934592\t17179869204\n" + b"x" * 300 + b"\t4\t5\nlast\t129\t150\n"
    rc, used, _ = _format_bed(SPAN, NAMES)
    assert (rc, used) == (N.KMAN_ECAP, len(want))
    rc, used, text = _format_bed(SPAN, NAMES, cap=len(want))
    assert (rc, used, text) == (N.KMAN_OK, len(want), want)
    rc, used, _ = _format_bed(SPAN, NAMES, cap=len(want) - 1)
    assert (rc, used) == (N.KMAN_ECAP, len(want))
    for keep in KEEPS:
        w = so.bed(recs, SPAN, keep)
        rc, used, text = _format_bed(SPAN, NAMES, keep, cap=len(w) + 16)
        assert (rc, used, text) == (N.KMAN_OK, len(w), w), keep
    assert so.bed(recs, SPAN, KEEPS[3]) == b""          # a kept record without a span: no line
    assert _format_bed([], [], cap=8) == (N.KMAN_OK, 0, b"")
    # an empty name with a span, END <= START never listed
    span = [(3, 9), (5, 5), (7, 6)]
    rc, used, text = _format_bed(span, [b"", b"b", b"c"], cap=64)
    assert (rc, text) == (N.KMAN_OK, b"\t3\t9\n")
    rng = np.random.default_rng(7)
    n = 20_000
    a = rng.integers(0, 1 << 20, n)
    span = list(zip(a.tolist(), (a + rng.integers(0, 3, n)).tolist()))
    names = [b"n%d" % i for i in range(n)]
    keep = rng.integers(0, 2, n).astype(np.uint8)
    w = so.bed([(x.decode(), "") for x in names], span, keep)
    for threads in (1, 4):
        rc, used, text = _format_bed(span, names, keep, cap=len(w), threads=threads)
        assert (rc, used) == (N.KMAN_OK, len(w)) and text == w


# ----------------------------------------------------------------------- CLI


@pytest.fixture()
def inputs(tmp_path):
    fa = tmp_path / "reads.fa"
    fa.write_bytes(b">r\nACGTACGTTGCAACGT\n")
    fb = tmp_path / "genome.fa"
    fb.write_bytes(b">s\nTTGCAACGTACG\n")
    return fa, fb


def test_help_shows_the_solid_options():
    from kman_amd.scripts.kmer import main

    text = CliRunner().invoke(main, ["screen", "--help"]).output
    for opt in ("--solid", "--min-solid-len", "--bed", "START", "END", "FILE"):
        assert opt in text, opt
    assert "breaks" in text and "exclusive" in text  # the coordinates: line breaks do not count, END is exclusive


REFUSED = {
    "solid_zero": (["5", "--solid", "0"], "--solid must be in [1, 4294967294]"),
    "solid_negative": (["5", "--solid=-2"], "--solid must be in [1, 4294967294]"),
    "solid_too_large": (["5", "--solid", "4294967295"], "--solid must be in [1, 4294967294]"),
    "len_without_solid": (["5", "--min-solid-len", "30"], "--min-solid-len needs --solid"),
    "len_negative": (["5", "--solid", "2", "--min-solid-len=-1"], "--min-solid-len must be >= 0"),
    "bed_without_solid": (["5", "--bed", "BED"], "--bed needs --solid"),
    "bed_with_median_only": (["5", "--median", "--bed", "BED"], "--bed needs --solid"),
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
    out, bed = tmp_path / "out.tsv", tmp_path / "out.bed"
    argv = [str(bed) if a == "BED" else a for a in argv]
    r = CliRunner().invoke(main, ["screen", str(inputs[0]), str(inputs[1]), str(out)] + argv)
    assert isinstance(r.exception, AssertionError), (r.exception, r.output)
    assert msg in str(r.exception)
    assert not out.exists() and not bed.exists()


def test_usage_errors(inputs, tmp_path):
    from kman_amd.scripts.kmer import main

    out = tmp_path / "out.tsv"
    for argv in (["5", "--solid", "x"], ["5", "--solid", "1.5"], ["5", "--solid"], ["5", "--solid", "2",
                                                                                   "--min-solid-len", "y"]):
        r = CliRunner().invoke(main, ["screen", str(inputs[0]), str(inputs[1]), str(out)] + argv)
        assert r.exit_code == 2 and not out.exists(), argv


@pytest.mark.parametrize("argv, median", [(["--solid", "3"], False), (["--solid", "4294967294", "--median"], True),
                                          (["--solid", "1", "--min-median", "2"], True)])
def test_solid_reaches_screen_solid(argv, median, inputs, tmp_path, monkeypatch):
    """--solid goes to engine.screen_solid with the threshold, never to screen / screen_median."""
    from kman_amd import engine
    from kman_amd.scripts import kmer

    class Reached(Exception):
        pass

    class _Table:
        pass

    class _Parsed:
        def free(self):
            pass

    def reached(p, table, canonical, min_count, **kw):
        raise Reached(min_count, kw.get("median"))

    def not_wanted(*a, **kw):
        raise RuntimeError("a screen without the runs")

    for v in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "KMAN_DIST"):
        monkeypatch.delenv(v, raising=False)
    monkeypatch.setattr(engine, "default_device", lambda *a, **kw: None)
    monkeypatch.setattr(engine, "parse_file", lambda *a, **kw: _Parsed())
    monkeypatch.setattr(engine, "check_empty_names", lambda *a, **kw: None)
    monkeypatch.setattr(engine, "join_groups", lambda *a, **kw: _Table())
    monkeypatch.setattr(engine, "free_result", lambda *a, **kw: None)
    monkeypatch.setattr(engine, "screen_solid", reached)
    monkeypatch.setattr(engine, "screen_median", not_wanted)
    monkeypatch.setattr(engine, "screen", not_wanted)
    out = tmp_path / "out.tsv"
    r = CliRunner().invoke(kmer.main, ["screen", str(inputs[0]), str(inputs[1]), str(out), "5"] + argv)
    assert isinstance(r.exception, Reached), (r.exception, r.output)
    assert r.exception.args == (int(argv[1]), median)
    assert not out.exists()


# ------------------------------------------------------------ plan, constants


def test_plan_call():
    from kman_amd import _native as N

    L = ctypes.CDLL(N.LIB_PATH)  # (host only: no device is asked for)
    fn = L.kman_record_runs_plan
    fn.restype, fn.argtypes = N.SIGNATURES["kman_record_runs_plan"]

    def plan(nb, nr):
        out = c_uint64(123)
        rc = fn(nb, nr, byref(out))
        return rc, out.value

    T = N.KMAN_RUNS_TILE
    rc, base = plan(0, 0)
    assert rc == N.KMAN_OK and 0 < base <= 4096 and base % 16 == 0
    assert plan(1, 1)[1] == plan(T, 1)[1] < plan(T + 1, 1)[1]      # by tiles
    assert plan(100 * T, 1)[1] == plan(100 * T, 10 ** 6)[1]         # not by records
    assert plan(1 << 28, 1)[1] <= (1 << 28) // 64                   # a small fraction of the words
    assert all(plan(n, 3)[1] % 16 == 0 for n in (1, T + 1, 7 * T, 1000 * T + 5))
    assert fn(0, 0, None) == N.KMAN_EINVAL
    assert plan(1 << 62, 1) == (N.KMAN_EINVAL, 0)


def test_header_signatures_and_constants_agree():
    from kman_amd import _native as N

    with open(os.path.join(os.path.dirname(N.HERE), "include", "kman.h")) as fh:
        text = fh.read()
    for name in ("KMAN_RUNS_TILE", "KMAN_RUNS_REC_CAP"):
        m = re.search(r"#define\s+%s\s+(\d+)\s" % name, text)
        assert m and int(m.group(1)) == getattr(N, name), name
    assert N.KMAN_RUNS_TILE == 4096 and N.KMAN_RUNS_TILE % 1024 == 0
    syms = N.header_symbols()
    for name, nargs in (("kman_record_runs_plan", 3), ("kman_record_runs", 9), ("kman_format_screen_solid", 12),
                        ("kman_format_bed", 10)):
        assert name in syms and name in N.SIGNATURES, name
        assert len(N.SIGNATURES[name][1]) == nargs, name
        decl = re.search(r"\bint %s\(([^;]*)\);" % name, text)
        assert decl and len(decl.group(1).split(",")) == nargs, name
    assert sorted(N.SIGNATURES) == syms
    assert re.search(r"#define\s+KMAN_ABI_VERSION\s+1\s", text)
    with open(os.path.join(N.HERE, "csrc", "runs.hip")) as fh:
        src = fh.read()
    for line in ("static_assert(RTILE == KMAN_RUNS_TILE", "constexpr int RCAP = KMAN_RUNS_REC_CAP"):
        assert line in src, line
    with open(os.path.join(N.HERE, "csrc", "Makefile")) as fh:
        assert "runs.hip" in fh.read()
