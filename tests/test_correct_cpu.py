"""`kmer screen --correct` without a GPU: the plain-Python statement
(tests/correct_cases.py) against hand-worked cases, the option refusals, the
ABI prototypes and bindings, and the host writer kman_format_screen_correct."""

from __future__ import annotations

import ctypes
import os
import re
from ctypes import byref, c_size_t, c_void_p

import numpy as np
import pytest
from click.testing import CliRunner

import correct_cases as cc
import median_cases as mc
import screen_cases as sc

NONE = mc.NONE


# ------------------------------------------------------------------- the rule


def test_site_rule_on_hand_built_words():
    k, C = 3, 2
    S, W = 5, 1  # a solid and a weak word
    # a record of 12 bases: window starts 0..9, the last two words NONE
    def words(ws):
        return ws + [NONE] * (k - 1)

    e = 12
    # L and R, a run of exactly k: the last window of the run starts at the wrong base
    w = words([S, S, W, W, W, S, S, S, S, S])
    assert cc.weak_runs(w, 0, e, C) == [(2, 5)] and cc.site_of(w, 2, 5, 0, e, k, C) == 4
    # L and R with another length: no site
    for run in ([S, S, W, W, S, S, S, S, S, S], [S, W, W, W, W, S, S, S, S, S]):
        (a, b), = cc.weak_runs(words(run), 0, e, C)
        assert cc.site_of(words(run), a, b, 0, e, k, C) is None
    # openL and R: at most k weak windows from the record's first base on
    assert cc.site_of(words([W, S, S, S, S, S, S, S, S, S]), 0, 1, 0, e, k, C) == 0
    assert cc.site_of(words([W, W, W, S, S, S, S, S, S, S]), 0, 3, 0, e, k, C) == 2
    assert cc.site_of(words([W, W, W, W, S, S, S, S, S, S]), 0, 4, 0, e, k, C) is None
    # L and openR: the run ends at the record's last window
    assert cc.site_of(words([S, S, S, S, S, S, S, S, S, W]), 9, 10, 0, e, k, C) == 11
    assert cc.site_of(words([S, S, S, S, S, S, S, W, W, W]), 7, 10, 0, e, k, C) == 9
    assert cc.site_of(words([S, S, S, S, S, S, W, W, W, W]), 6, 10, 0, e, k, C) is None
    # both sides open; a NONE neighbour on either side
    assert cc.site_of(words([W] * 10), 0, 10, 0, e, k, C) is None
    assert cc.site_of(words([S, NONE, W, W, W, S, S, S, S, S]), 2, 5, 0, e, k, C) is None
    assert cc.site_of(words([S, S, W, W, W, NONE, S, S, S, S]), 2, 5, 0, e, k, C) is None
    # the threshold: C - 1 is weak, C is solid
    assert cc.weak(C - 1, C) and not cc.weak(C, C) and cc.solid(C, C) and not cc.solid(C - 1, C)
    assert not cc.weak(NONE, C) and not cc.solid(NONE, C)
    # a run is cut at its record's ends: two records of 6 and 6 bases
    w = [S, W, W, W, NONE, NONE, W, W, S, S, NONE, NONE]
    assert cc.weak_runs(w, 0, 6, C) == [(1, 4)] and cc.weak_runs(w, 6, 12, C) == [(6, 8)]
    assert cc.named_sites(w, [0, 6], 12, k, C) == [3, 7]  # L and openR (p = 1 + 3 - 1), openL and R (p = 8 - 1)


@pytest.mark.parametrize("k, canonical", [(3, False), (4, False), (4, True)])
def test_statement_on_the_hand_cases(k, canonical):
    cases = cc.hand_cases(k, canonical)
    names = [c[0] for c in cases]
    for want in ("interior", "first_base", "last_base", "column_k_minus_1", "column_e_minus_k",
                 "two_more_than_k_apart", "two_exactly_k_apart", "two_closer_than_k", "two_alternatives_ok",
                 "no_alternative_ok", "run_touching_an_N", "record_of_k_bases", "short_and_empty_records", "count_C",
                 "count_C_minus_1", "candidate_window_at_C_minus_1"):
        assert want in names
    for name, recs, table, C, expected in cases:
        n = sum(len(s) for _, s in recs)
        got = cc.fix_plane_of(recs, k, table, C, canonical)
        assert got == cc.expected_plane(n, expected), name
        fixed = cc.corrected(recs, got)
        if name in ("interior", "first_base", "last_base", "column_k_minus_1", "column_e_minus_k",
                    "two_more_than_k_apart", "count_C"):
            assert len(expected) >= 1 and fixed[0][1] == cc.hand_genome(k), name  # the read is the genome again
        if name == "short_and_empty_records":
            assert cc.nfix(got, sc.codes_of(recs)[1], n) == [1, 0, 0, 0, 0, 1, 0]
    # the weak runs are the ones the cases were built for (two errors exactly k apart: one run of 2 k)
    runs = cc.hand_runs(k)
    assert runs["two_exactly_k_apart"] == [(2, 2 * k + 2)]
    for name, recs, table, C, _ in cases:
        if name in runs:
            words = mc.window_words(recs, k, table, canonical)
            assert cc.weak_runs(words, 0, len(words), C) == runs[name], name


def test_a_masked_base_is_an_N():
    """A base that -q masks has the code of an N: the run beside it names no site."""
    from fastq_qual_cases import mask_fastq

    k = 4
    g = cc.hand_genome(k)
    m = 2 * k
    read = cc.sub(g, m)
    qual = "I" * (m + k) + "#" + "I" * (len(g) - m - k - 1)
    fasta, n_masked = mask_fastq(("@r\n%s\n+\n%s\n" % (read, qual)).encode(), 20, 33)
    recs = sc.fasta_records(fasta)
    assert n_masked == 1 and recs[0][1][m + k] == "N"
    table = cc.kmer_table([g], k)
    assert cc.fix_plane_of(recs, k, table, 3) == [cc.NOFIX] * len(g)
    assert cc.fix_plane_of([("r", read)], k, table, 3)[m] == "ACGT".index(g[m])  # fixed without the mask


def test_random_case_has_a_repaired_read_and_a_site_left_alone():
    k, C = 15, 3
    genome, reads, clean = cc.random_case()
    table = cc.kmer_table([genome], k)
    fix = cc.fix_plane_of(reads, k, table, C)
    fixed = cc.corrected(reads, fix)
    assert any(r != c and f == c for r, c, f in zip(reads, clean, fixed))  # a read with errors, fully repaired
    _, rec_seq, n = sc.codes_of(reads)
    sites = cc.named_sites(mc.window_words(reads, k, table), rec_seq, n, k, C)
    assert any(fix[p] == cc.NOFIX for p in sites) and any(fix[p] != cc.NOFIX for p in sites)
    assert sum(1 for f in fix if f != cc.NOFIX) == sum(cc.nfix(fix, rec_seq, n))


def test_apply_statement():
    codes = [8 | 1, 2, 4, 3, 8 | 0, 0]
    fix = [3, cc.NOFIX, cc.NOFIX, 0, 2, cc.NOFIX]
    assert cc.apply_codes(codes, fix) == [8 | 3, 2, 4, 0, 8 | 2, 0]
    assert cc.nfix(fix, [0, 4], 6) == [2, 1] and cc.nfix(fix, [0, 0, 4, 6, 9], 6) == [0, 2, 1, 0, 0]
    # "\r\n", a blank inside the sequence line (it shifts the code index), a lower-case base, trailing blanks
    text = b"@a x\r\nAC gT \r\n+\r\nIIIII\r\n@b\nacgt\n+\n!!!!\n"
    want = b"@a x\r\nTC gA \r\n+\r\nIIIII\r\n@b\ngcgt\n+\n!!!!\n"
    got = cc.apply_text(text, [0, text.index(b"@b"), len(text)], [0, 4], [3, cc.NOFIX, cc.NOFIX, 0, 2, 255, 255, 255], 8)
    assert got == want


# ----------------------------------------------------------------------- CLI


@pytest.fixture()
def inputs(tmp_path):
    fa = tmp_path / "reads.fa"
    fa.write_bytes(b">r\nACGTACGTTGCAACGT\n")
    fq = tmp_path / "reads.fq"
    fq.write_bytes(b"@r\nACGTACGTTGCAACGT\n+\nIIIIIIIIIIIIIIII\n")
    fb = tmp_path / "genome.fa"
    fb.write_bytes(b">s\nTTGCAACGTACG\n")
    return fa, fb, fq


REFUSED = {
    "correct_without_solid": ("fa", ["5", "--correct"], "--correct needs --solid"),
    "correct_with_median_only": ("fq", ["5", "--correct", "--median"], "--correct needs --solid"),
    "fasta_with_reads_out": ("fa", ["5", "--solid", "2", "--correct", "--reads-out", "READS"],
                             "--correct with --reads-out needs fastq READS"),
    "forced_fasta_with_reads_out": ("fq", ["5", "--solid", "2", "--correct", "--reads-out", "READS", "--format",
                                           "fasta"], "--correct with --reads-out needs fastq READS"),
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
    which, argv, msg = REFUSED[case]
    out, reads = tmp_path / "out.tsv", tmp_path / "out.fq"
    argv = [str(reads) if a == "READS" else a for a in argv]
    src = inputs[0] if which == "fa" else inputs[2]
    r = CliRunner().invoke(main, ["screen", str(src), str(inputs[1]), str(out)] + argv)
    assert isinstance(r.exception, AssertionError), (r.exception, r.output)
    assert msg in str(r.exception)
    assert not out.exists() and not reads.exists()


def test_help_and_other_commands():
    from kman_amd.scripts.kmer import main

    text = CliRunner().invoke(main, ["screen", "--help"]).output
    assert "--correct" in text and "FIXES" in text
    assert "--correct" not in CliRunner().invoke(main, ["classify", "--help"]).output


@pytest.mark.parametrize("argv, want", [(["--solid", "3", "--correct"], True), (["--solid", "3"], False)])
def test_correct_runs_before_the_screen(argv, want, inputs, tmp_path, monkeypatch):
    """--correct calls engine.correct with --solid's threshold before screen_solid; without it, never."""
    from kman_amd import engine
    from kman_amd.scripts import kmer

    class Reached(Exception):
        pass

    class _Parsed:
        def free(self):
            pass

    calls = []

    def correct(p, table, canonical, min_count, **kw):
        calls.append(("correct", min_count))
        return np.zeros(0, np.uint32)

    def solid(p, table, canonical, min_count, **kw):
        calls.append(("solid", min_count))
        raise Reached()

    for v in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "KMAN_DIST"):
        monkeypatch.delenv(v, raising=False)
    monkeypatch.setattr(engine, "default_device", lambda *a, **kw: None)
    monkeypatch.setattr(engine, "parse_file", lambda *a, **kw: _Parsed())
    monkeypatch.setattr(engine, "check_empty_names", lambda *a, **kw: None)
    monkeypatch.setattr(engine, "join_groups", lambda *a, **kw: object())
    monkeypatch.setattr(engine, "free_result", lambda *a, **kw: None)
    monkeypatch.setattr(engine, "correct", correct)
    monkeypatch.setattr(engine, "screen_solid", solid)
    out = tmp_path / "out.tsv"
    r = CliRunner().invoke(kmer.main, ["screen", str(inputs[0]), str(inputs[1]), str(out), "5"] + argv)
    assert isinstance(r.exception, Reached), (r.exception, r.output)
    assert calls == ([("correct", 3)] if want else []) + [("solid", 3)]


# ------------------------------------------------------------ ABI, the writer


def test_header_signatures_and_constants_agree():
    from kman_amd import _native as N

    with open(os.path.join(os.path.dirname(N.HERE), "include", "kman.h")) as fh:
        text = fh.read()
    for name in ("KMAN_CORRECT_TILE", "KMAN_CORRECT_REC_CAP"):
        m = re.search(r"#define\s+%s\s+(\d+)\s" % name, text)
        assert m and int(m.group(1)) == getattr(N, name), name
    assert re.search(r"#define\s+KMAN_FIX_NONE\s+0xFFu\s", text) and N.KMAN_FIX_NONE == 0xFF == cc.NOFIX
    syms = N.header_symbols()
    for name, nargs in (("kman_correct_sites", 17), ("kman_apply_fixes", 10), ("kman_format_screen_correct", 13)):
        assert name in syms and name in N.SIGNATURES, name
        assert len(N.SIGNATURES[name][1]) == nargs, name
        decl = re.search(r"\bint %s\(([^;]*)\);" % name, text)
        assert decl and len(decl.group(1).split(",")) == nargs, name
        assert hasattr(ctypes.CDLL(N.LIB_PATH), name), name
    assert sorted(N.SIGNATURES) == syms
    assert re.search(r"#define\s+KMAN_ABI_VERSION\s+1\s", text)
    with open(os.path.join(N.HERE, "csrc", "correct.hip")) as fh:
        src = fh.read()
    for line in ("constexpr int CTILE = KMAN_CORRECT_TILE", "constexpr int CCAP = KMAN_CORRECT_REC_CAP",
                 "table_lookup<1, CT>"):
        assert line in src, line
    with open(os.path.join(N.HERE, "csrc", "Makefile")) as fh:
        assert "correct.hip" in fh.read()


def _format_correct(st, med, span, fixes, names, keep=None, cap=0, threads=2):
    from kman_amd import _native as N

    L = ctypes.CDLL(N.LIB_PATH)  # (host only: no device is asked for)
    fn = L.kman_format_screen_correct
    fn.restype, fn.argtypes = N.SIGNATURES["kman_format_screen_correct"]
    R = len(names)
    planes = np.ascontiguousarray(np.asarray(st, dtype=np.uint64).reshape(-1, 3).T)
    start = np.ascontiguousarray([s[0] for s in span], dtype=np.uint64)
    end = np.ascontiguousarray([s[1] for s in span], dtype=np.uint64)
    fx = np.ascontiguousarray(fixes, dtype=np.uint32)
    m = np.ascontiguousarray(med, dtype=np.uint32) if med is not None else None
    off = np.concatenate([[0], np.cumsum([len(n) for n in names])]).astype(np.uint64)
    kp = np.ascontiguousarray(keep, dtype=np.uint8) if keep is not None else None
    buf = ctypes.create_string_buffer(max(1, cap)) if cap else None
    used = c_size_t(0)
    rc = fn(planes.ctypes.data_as(c_void_p), m.ctypes.data_as(c_void_p) if m is not None else None,
            start.ctypes.data_as(c_void_p), end.ctypes.data_as(c_void_p), fx.ctypes.data_as(c_void_p), R,
            kp.ctypes.data_as(c_void_p) if kp is not None else None, b"".join(names), off.ctypes.data_as(c_void_p), buf,
            cap, byref(used), threads)
    return rc, used.value, (buf.raw[:used.value] if buf is not None and rc == 0 else b"")


NAMES = [b"with\ttab", b"", b"r/1", b"x" * 300, b"last"]
ST = [(5, 5, (1 << 32) + 7), (0, 0, 0), (1 << 40, 3, (1 << 64) - 1), (9, 0, 0), (7, 7, 7)]
MED = [4294967294, 0, 17, 1, 7]
SPAN = [(0, 25), (0, 0), (1 << 33, (1 << 34) + 20), (4, 5), (129, 150)]
FIXES = [0, 3, 4294967295, 10, 1]


@pytest.mark.parametrize("with_median", [False, True])
def test_format_screen_correct(with_median):
    from kman_amd import _native as N

    med = MED if with_median else None
    recs = [(n.decode(), "") for n in NAMES]
    want = cc.lines(recs, ST, SPAN, FIXES, med)
    if with_median:
        assert b"with\ttab\t5\t5\t4294967303\t4294967294\t0\t25\t0\n" in want and b"\n\t0\t0\t0\t0\t0\t0\t3\n" in want
    else:
        assert b"with\ttab\t5\t5\t4294967303\t0\t25\t0\n" in want and b"last\t7\t7\t7\t129\t150\t1\n" in want
        assert b"\t17179869204\t4294967295\n" in want
    rc, used, _ = _format_correct(ST, med, SPAN, FIXES, NAMES)  # sizing call: no buffer
    assert (rc, used) == (N.KMAN_ECAP, len(want))
    rc, used, text = _format_correct(ST, med, SPAN, FIXES, NAMES, cap=len(want))
    assert (rc, used, text) == (N.KMAN_OK, len(want), want)
    rc, used, _ = _format_correct(ST, med, SPAN, FIXES, NAMES, cap=len(want) - 1)  # one byte short: the size reported
    assert (rc, used) == (N.KMAN_ECAP, len(want))
    for keep in ([1, 0, 1, 0, 0], [0] * 5, [1] * 5, [0, 2, 0, 255, 0]):
        w = cc.lines(recs, ST, SPAN, FIXES, med, keep)
        rc, used, text = _format_correct(ST, med, SPAN, FIXES, NAMES, keep, cap=len(w) + 16)
        assert (rc, used, text) == (N.KMAN_OK, len(w), w), keep
    assert _format_correct([], [] if with_median else None, [], [], [], cap=8) == (N.KMAN_OK, 0, b"")
    rng = np.random.default_rng(8)
    n = 20_000
    st = rng.integers(0, 1 << 40, (n, 3), dtype=np.uint64)
    m = rng.integers(0, 1 << 32, n, dtype=np.uint64) if with_median else None
    a = rng.integers(0, 1 << 20, n)
    span = list(zip(a.tolist(), (a + rng.integers(0, 300, n)).tolist()))
    fx = rng.integers(0, 200, n)
    names = [b"n%d" % i for i in range(n)]
    keep = rng.integers(0, 2, n).astype(np.uint8)
    w = cc.lines([(x.decode(), "") for x in names], st, span, fx, m, keep)
    for threads in (1, 4):
        rc, used, text = _format_correct(st, m, span, fx, names, keep, cap=len(w), threads=threads)
        assert (rc, used) == (N.KMAN_OK, len(w)) and text == w


def test_emit_screen_default_is_todays_call(monkeypatch):
    """emit_screen without fixes= calls the writers it called before; with it, the new one."""
    from kman_amd import engine
    from kman_amd.engine import Parsed

    names = [b"a", b"bb"]
    p = Parsed(None, None, 30, 2, np.array([0, 9], np.uint64), np.array([0, 10], np.uint64), names, b"".join(names),
               np.array([0, 1, 3], np.uint64))
    st = np.array([[5, 4, 9], [7, 0, 0]], np.uint64)
    span = (np.array([0, 2], np.uint64), np.array([9, 2], np.uint64))
    recs = [("a", ""), ("bb", "")]
    import solid_cases as so

    pairs = [(0, 9), (2, 2)]
    assert engine.emit_screen(p, st, None, span=span) == so.lines(recs, st, pairs)
    assert engine.emit_screen(p, st, None, span=span, fixes=None) == so.lines(recs, st, pairs)
    assert engine.emit_screen(p, st, None, span=span, fixes=[2, 0]) == cc.lines(recs, st, pairs, [2, 0])
    assert engine.emit_screen(p, st, [0, 1], median=[3, 4], span=span, fixes=[2, 0]) == \
        cc.lines(recs, st, pairs, [2, 0], [3, 4], [0, 1])
    with pytest.raises(AssertionError):
        engine.emit_screen(p, st, None, fixes=[2, 0])          # no span
    with pytest.raises(AssertionError):
        engine.emit_screen(p, st, None, span=span, fixes=[2])  # one word per record
