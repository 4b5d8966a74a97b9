"""`kmer screen` without a GPU: the command's options, every refusal raised
before any device work or output file, the ABI's constants and signatures,
the host formatter kman_format_screen, engine.screen_keep, and the
plain-Python statement (tests/screen_cases.py) pinned to a hand-written
example."""

from __future__ import annotations

import ctypes
import os
import re
from ctypes import byref, c_size_t, c_void_p

import numpy as np
import pytest
from click.testing import CliRunner

import screen_cases as sc


@pytest.fixture()
def inputs(tmp_path):
    fa = tmp_path / "reads.fa"
    fa.write_bytes(b">r\nACGTACGTTGCAACGT\n")
    fb = tmp_path / "genome.fa"
    fb.write_bytes(b">s\nTTGCAACGTACG\n")
    fq = tmp_path / "reads.fq"
    fq.write_bytes(b"@q\nACGTACGTTG\n+\nIIIIIIIIII\n")
    return fa, fb, fq


def test_help_shows_every_option():
    from kman_amd.scripts.kmer import main

    run = CliRunner()
    text = run.invoke(main, ["screen", "--help"]).output
    for opt in ("READS", "TABLE_INPUT", "OUTPUT", " K", "--canonical", "--format", "-q,", "--min-qual",
                "--phred-offset", "-L,", "--min-count", "-U,", "--max-count", "--min-hits", "--min-frac", "-v",
                "--invert", "--index-bits", "Not part of the reference"):
        assert opt in text, opt
    assert "-r," not in text and "--reverse" not in text
    assert "screen" in run.invoke(main, ["--help"]).output


REFUSED = {
    "k_1": (["1"], "k must be >= 1"),
    "k_33": (["33"], "K <= 32"),
    "k_40": (["40"], "stated limit"),
    "min_above_max": (["5", "-L", "6", "-U", "5"], "--min-count 6 is greater than --max-count 5"),
    "min_frac_above_1": (["5", "--min-frac", "1.5"], "--min-frac"),
    "min_frac_negative": (["5", "--min-frac=-0.1"], "--min-frac"),
    "min_frac_nan": (["5", "--min-frac", "nan"], "--min-frac"),
    "min_hits_negative": (["5", "--min-hits=-1"], "--min-hits"),
    "min_qual_without_fastq": (["5", "-q", "20"], "--min-qual"),
    "index_bits_above_2k": (["5", "--index-bits", "11"], "--index-bits"),
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


@pytest.mark.parametrize("argv", [[], ["5", "--index-bits", "0"], ["5", "--index-bits", "25"], ["5", "-L", "0"],
                                  ["5", "--min-frac", "half"], ["5", "-r"]])
def test_usage_errors(argv, inputs, tmp_path):
    from kman_amd.scripts.kmer import main

    out = tmp_path / "out.tsv"
    r = CliRunner().invoke(main, ["screen", str(inputs[0]), str(inputs[1]), str(out)] + argv)
    assert r.exit_code == 2 and not out.exists()


def test_min_qual_is_taken_when_one_input_is_fastq(inputs, tmp_path, monkeypatch):
    from kman_amd import engine
    from kman_amd.scripts.kmer import main

    class Reached(Exception):
        pass

    def device(*a, **kw):
        raise Reached()

    monkeypatch.setattr(engine, "default_device", device)
    for v in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "KMAN_DIST"):
        monkeypatch.delenv(v, raising=False)
    out = tmp_path / "out.tsv"
    for a, b in ((inputs[2], inputs[1]), (inputs[0], inputs[2])):
        r = CliRunner().invoke(main, ["screen", str(a), str(b), str(out), "5", "-q", "20"])
        assert isinstance(r.exception, Reached), (r.exception, r.output)
    r = CliRunner().invoke(main, ["screen", str(inputs[2]), str(inputs[1]), str(out), "5", "-q", "20", "--format",
                                  "fasta"])
    assert isinstance(r.exception, AssertionError) and "--min-qual" in str(r.exception)
    assert not out.exists()


def test_runs_on_rank_0_alone(inputs, tmp_path, monkeypatch):
    from kman_amd import engine
    from kman_amd.scripts.kmer import main

    def no_device(*a, **kw):
        raise RuntimeError("a rank other than 0 asked for the device")

    monkeypatch.setattr(engine, "default_device", no_device)
    monkeypatch.setenv("WORLD_SIZE", "4")
    monkeypatch.setenv("RANK", "2")
    monkeypatch.setenv("LOCAL_RANK", "2")
    monkeypatch.delenv("KMAN_DIST", raising=False)
    out = tmp_path / "out.tsv"
    r = CliRunner().invoke(main, ["screen", str(inputs[0]), str(inputs[1]), str(out), "5"])
    assert r.exception is None and r.exit_code == 0 and not out.exists()
    r = CliRunner().invoke(main, ["screen", str(inputs[0]), str(inputs[1]), str(out), "40"])  # (refused on every rank)
    assert isinstance(r.exception, AssertionError)


def test_header_signatures_and_constants_agree():
    from kman_amd import _native as N

    with open(os.path.join(os.path.dirname(N.HERE), "include", "kman.h")) as fh:
        text = fh.read()
    for name in ("KMAN_SCREEN_MAX_INDEX_BITS", "KMAN_SCREEN_TILE", "KMAN_SCREEN_REC_CAP"):
        m = re.search(r"#define\s+%s\s+(\d+)\s" % name, text)
        assert m and int(m.group(1)) == getattr(N, name), name
    assert N.KMAN_SCREEN_MAX_INDEX_BITS == 24
    assert N.KMAN_SCREEN_TILE % N.KMAN_SCREEN_REC_CAP == 0
    syms = N.header_symbols()
    for name, nargs in (("kman_table_index", 6), ("kman_screen_records", 14), ("kman_format_screen", 9)):
        assert name in syms and name in N.SIGNATURES, name
        assert len(N.SIGNATURES[name][1]) == nargs, name
        decl = re.search(r"\bint %s\(([^;]*)\);" % name, text)
        assert decl and len(decl.group(1).split(",")) == nargs, name
    assert sorted(N.SIGNATURES) == syms
    assert re.search(r"#define\s+KMAN_ABI_VERSION\s+1\s", text)
    with open(os.path.join(N.HERE, "csrc", "screen.hip")) as fh:
        src = fh.read()
    assert "static_assert(STILE == KMAN_SCREEN_TILE" in src and "SCAP = KMAN_SCREEN_REC_CAP" in src
    with open(os.path.join(N.HERE, "csrc", "Makefile")) as fh:
        assert "screen.hip" in fh.read()


def test_default_index_bits():
    from kman_amd import engine

    want = {0: 1, 1: 1, 2: 1, 16: 1, 17: 2, 1 << 20: 17, (1 << 20) + 1: 18, 10 ** 9: 24}
    for n, bits in want.items():
        assert engine.default_index_bits(n, 21) == bits, n
    assert engine.default_index_bits(10 ** 9, 5) == 10 and engine.default_index_bits(10 ** 6, 2) == 4
    assert "nobody has measured" in " ".join(engine.table_index.__doc__.split())


# ------------------------------------------------------------ host formatter


def _format_screen(st, names, keep=None, cap=None, threads=3):
    """(return code, used, text) of one kman_format_screen call."""
    from kman_amd import _native as N

    L = ctypes.CDLL(N.LIB_PATH)  # (the formatter is host code: no device is asked for)
    fn = L.kman_format_screen
    fn.restype, fn.argtypes = N.SIGNATURES["kman_format_screen"]
    st = np.asarray(st, dtype=np.uint64).reshape(-1, 3)
    n = st.shape[0]
    planes = np.ascontiguousarray(st.T)
    blob = b"".join(names)
    off = np.zeros(n + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(x) for x in names])
    kp = None
    if keep is not None:
        keep = np.asarray(keep, dtype=np.uint8)
        kp = keep.ctypes.data_as(c_void_p)
    used = c_size_t(0)
    buf = ctypes.create_string_buffer(max(1, cap)) if cap is not None else None
    rc = fn(planes.ctypes.data_as(c_void_p), n, kp, blob, off.ctypes.data_as(c_void_p), buf, cap or 0, byref(used),
            threads)
    return rc, used.value, (buf.raw[:used.value] if buf is not None and rc == 0 else None)


def _want_lines(st, names, keep=None):
    return b"".join(nm + b"\t%d\t%d\t%d\n" % tuple(int(x) for x in row)
                    for r, (nm, row) in enumerate(zip(names, st)) if keep is None or keep[r])


def test_format_screen():
    from kman_amd import _native as N

    big = (1 << 64) - 1
    st = [(136, 0, 0), (0, 0, 0), (5, 5, (1 << 32) + 7), (1 << 33, (1 << 32) + 1, big), (10, 3, 999), (7, 7, 7)]
    names = [b"read1", b"", b"with\ttab", b"r/1", b"x" * 300, b"last"]
    want = _want_lines(st, names)
    rc, used, _ = _format_screen(st, names)  # sizing call: no buffer
    assert (rc, used) == (N.KMAN_ECAP, len(want))
    rc, used, text = _format_screen(st, names, cap=len(want))
    assert (rc, used, text) == (N.KMAN_OK, len(want), want)
    rc, used, _ = _format_screen(st, names, cap=len(want) - 1)  # one byte short: refused, the size reported
    assert (rc, used) == (N.KMAN_ECAP, len(want))
    for keep in ([1, 0, 1, 0, 0, 1], [0] * 6, [1] * 6, [0, 0, 0, 1, 0, 0], [0, 2, 0, 0, 255, 0]):
        w = _want_lines(st, names, keep)
        rc, used, text = _format_screen(st, names, keep, cap=len(w) + 16)
        assert (rc, used, text) == (N.KMAN_OK, len(w), w), keep
    rc, used, text = _format_screen([], [], cap=8)  # zero records
    assert (rc, used, text) == (N.KMAN_OK, 0, b"")
    # many records over several host threads
    rng = np.random.default_rng(5)
    n = 20_000
    st = rng.integers(0, 1 << 40, (n, 3), dtype=np.uint64)
    names = [b"n%d" % i for i in range(n)]
    keep = rng.integers(0, 2, n).astype(np.uint8)
    w = _want_lines(st, names, keep)
    for threads in (1, 4):
        rc, used, text = _format_screen(st, names, keep, cap=len(w), threads=threads)
        assert (rc, used) == (N.KMAN_OK, len(w)) and text == w


def test_screen_keep_on_hand_written_rows():
    from kman_amd import engine

    #            windows hits sum
    st = np.asarray([(10, 0, 0), (10, 5, 9), (10, 10, 30), (0, 0, 0), (3, 1, 1), (4, 2, 1 << 40)], dtype=np.uint64)
    cases = [
        ((0, 0.0, False), [1, 1, 1, 1, 1, 1]),
        ((1, 0.0, False), [0, 1, 1, 0, 1, 1]),
        ((0, 1.0, False), [0, 0, 1, 1, 0, 0]),   # windows == 0: 0 >= 1.0 * 0
        ((0, 0.5, False), [0, 1, 1, 1, 0, 1]),
        ((1, 1.0, False), [0, 0, 1, 0, 0, 0]),
        ((2, 0.5, False), [0, 1, 1, 0, 0, 1]),
        ((6, 0.0, False), [0, 0, 1, 0, 0, 0]),
        ((1, 0.0, True), [1, 0, 0, 1, 0, 0]),
        ((0, 0.0, True), [0, 0, 0, 0, 0, 0]),
        ((0, 1.0, True), [1, 1, 0, 0, 1, 1]),
    ]
    for (mh, mf, inv), want in cases:
        got = engine.screen_keep(st, mh, mf, inv)
        assert got.dtype == np.uint8 and got.tolist() == want, (mh, mf, inv)
        assert [int(x) for x in sc.keep(st, mh, mf, inv)] == want, (mh, mf, inv)
    assert engine.screen_keep(np.zeros((0, 3), np.uint64)).shape == (0,)


def test_helper_on_a_six_read_example():
    """k = 3, written out by hand."""
    genome = [("g1", "ACGTAC"), ("g2", "acgNTTT")]
    # forward 3-mers: ACG x2 (g1, g2), CGT, GTA, TAC, TTT
    table = sc.table_of(genome, 3)
    assert table == {"ACG": 2, "CGT": 1, "GTA": 1, "TAC": 1, "TTT": 1}
    reads = [
        ("all", "ACGTA"),       # ACG CGT GTA: 3 windows, 3 hits, 2 + 1 + 1
        ("none", "GGGGG"),      # 3 windows, none in the table
        ("short", "AC"),        # no window
        ("empty", ""),
        ("masked", "ACGNTTTn"),  # ACG, TTT valid (CGN GNT NTT TTn are not): 2 hits, 2 + 1
        ("lower", "ttta"),      # TTT, TTA: 1 hit
    ]
    want = [(3, 3, 4), (3, 0, 0), (0, 0, 0), (0, 0, 0), (2, 2, 3), (2, 1, 1)]
    assert sc.stats(reads, 3, table).tolist() == [list(x) for x in want]
    # canonical: ACG/CGT -> ACG, GTA/TAC -> GTA, TTT -> AAA
    ctable = sc.table_of(genome, 3, canonical=True)
    assert ctable == {"ACG": 3, "GTA": 2, "AAA": 1}
    cwant = [(3, 3, 8), (3, 0, 0), (0, 0, 0), (0, 0, 0), (2, 2, 4), (2, 1, 1)]
    assert sc.stats(reads, 3, ctable, canonical=True).tolist() == [list(x) for x in cwant]
    assert sc.table_of(genome, 3, min_count=2) == {"ACG": 2}
    kept = sc.keep(np.asarray(want), 1, 0.6)
    assert kept == [True, False, False, False, True, False]
    assert sc.lines(reads, np.asarray(want), kept) == b"all\t3\t3\t4\nmasked\t2\t2\t3\n"
    assert sc.lines(reads, np.asarray(want)).count(b"\n") == 6
    keys, counts = sc.table_rows(table)
    assert keys.tolist() == [0b000110, 0b011011, 0b101100, 0b110001, 0b111111] and counts.tolist() == [2, 1, 1, 1, 1]
    codes, rec_seq, n = sc.codes_of(reads)
    assert n == 24 and rec_seq.tolist() == [0, 5, 10, 12, 12, 20] and len(codes) == n + 64
    assert codes[:6].tolist() == [8, 1, 2, 3, 0, 10] and codes[15] == 4 and codes[19] == 4 and codes[n:].tolist() == [4] * 64
    assert sc.fasta_records(sc.fasta(reads)) == reads
