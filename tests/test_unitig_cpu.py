"""`kmer unitigs` without a GPU: the plain-Python statement
(tests/unitig_cases.py) held to its two checkers on every named case and
pinned to hand-written outputs, the host formatter against the statement, the
ABI section's text and signatures, and every refusal of the command, raised
before any device work or output file."""

from __future__ import annotations

import os
import re

import numpy as np
import pytest
from click.testing import CliRunner

import unitig_cases as uc

CASES = uc.cases()


@pytest.mark.parametrize("name", sorted(CASES))
def test_statement_passes_both_checkers(name):
    records, k, min_count = CASES[name]
    base = uc.table_of(records, k, min_count)
    for v, recs in enumerate((records, uc.both_strands(records), uc.reverse_strand(records))):
        table = uc.table_of(recs, k, 2 * min_count - 1 if v == 1 else min_count)
        assert sorted(table) == sorted(base)
        units = uc.unitigs(table)
        assert [(s, m) for s, m, _ in units] == [(s, m) for s, m, _ in uc.unitigs(base)]  # counts aside
        assert all(len(s) == m + k - 1 for s, m, _ in units)
        assert sum(c for _, _, c in units) == sum(table.values())
        if table:
            uc.check_cover([s for s, _, _ in units], table, k)
            uc.check_maximal([s for s, _, _ in units], table, k)
        assert uc.parse_text(uc.text(units), k) == units
        link = uc.links(table)
        assert all(link[v_] == u for u, v_ in link.items())  # links are symmetric
        starts = [w[0][0] for w in uc.walks(table)[0]]
        assert starts == sorted(starts)  # file order
    if name.startswith(("path_", "cycle_")) and "_with_" not in name:
        assert len(uc.unitigs(base)) == 1 and len(base) == int(name.split("_")[1])


def test_the_checkers_refuse_wrong_unitigs():
    records, k, _ = CASES["y_fork"]
    table = uc.table_of(records, k)
    seqs = [s for s, _, _ in uc.unitigs(table)]
    longest = max(seqs, key=len)
    rest = [s for s in seqs if s is not longest]
    split = rest + [longest[:k + 5], longest[6:]]  # still a cover, no longer maximal
    uc.check_cover(split, table, k)
    with pytest.raises(AssertionError):
        uc.check_maximal(split, table, k)
    with pytest.raises(AssertionError):
        uc.check_cover(rest, table, k)  # k-mers missing
    with pytest.raises(AssertionError):
        uc.check_cover(seqs + [longest], table, k)  # k-mers twice
    merged = [records[0][1]] + [s for s in seqs if uc.canon(s[:k]) not in
                                {uc.canon(records[0][1][i:i + k]) for i in range(len(records[0][1]) - k + 1)}]
    uc.check_cover(merged, table, k)
    with pytest.raises(AssertionError):
        uc.check_maximal(merged, table, k)  # a junction through the fork is no link


def test_hand_written_outputs():
    def out(records, k, **kw):
        return uc.text(uc.unitigs(uc.table_of(records, k, **kw)))

    # ACG and CGT are one canonical k-mer whose only neighbour is itself: it never joins through that side
    assert out([("h", "ACGT")], 3) == b">0 LN:i:3 KC:i:2\nACG\n"
    # poly-A: AAA follows itself
    assert out([("a", "AAAAAAA")], 3) == b">0 LN:i:3 KC:i:5\nAAA\n"
    assert out([("a", "AAAAAAA"), ("t", "TTTT")], 3) == b">0 LN:i:3 KC:i:7\nAAA\n"
    # a 2-node cycle: ACACA -> CACAC -> ACACA; cut at side L of ACACA, spelled from there
    assert out([("c", "ACACAC")], 5) == b">0 LN:i:6 KC:i:2\nACACAC\n"
    assert out([("c", "ACACACACA")], 5) == b">0 LN:i:6 KC:i:5\nACACAC\n"
    assert out([("c", "GTGTGT")], 5) == b">0 LN:i:6 KC:i:2\nACACAC\n"  # the other strand: the same file
    # a Y-fork at k = 3: CAA -> AAG, then AGA or AGC.  Rows AAG 0, AGA 1, AGC 2, CAA 3; side R of AAG has two
    # neighbours, so AGA and AGC stay alone; AAG joins CAA through its side L and is the smaller end: the path
    # leaves AAG through L, spelled CTT, then TTG = revcomp(CAA) adds G.  AGC's right neighbour GCT is itself.
    assert out([("s_a", "CAAGA"), ("s_b", "CAAGC")], 3) == (b">0 LN:i:4 KC:i:4\nCTTG\n"
                                                            b">1 LN:i:3 KC:i:1\nAGA\n"
                                                            b">2 LN:i:3 KC:i:1\nAGC\n")
    assert uc.link_array(uc.table_of([("s_a", "CAAGA"), ("s_b", "CAAGC")], 3)).tolist() == [
        uc.NONE, (3 << 1) | uc.R, uc.NONE, uc.NONE, uc.NONE, uc.NONE, (0 << 1) | uc.L, uc.NONE]
    start, pos, nodes = uc.rank_arrays(uc.table_of([("s_a", "CAAGA"), ("s_b", "CAAGC")], 3))
    assert start.tolist() == [0, 1, 2, 0] and pos.tolist() == [1, 0, 0, 3] and nodes.tolist() == [2, 1, 1, 0]
    # -L 2 drops the branch that was seen once: rows AAG 0 (3), AGA 1 (2), CAA 2 (3), one path whose ends are
    # AGA and CAA; it starts at AGA, the smaller row, which is left through L: the text is revcomp(CAAGA)
    assert out([("s_a", "CAAGA"), ("s_a2", "CAAGA"), ("s_b", "CAAGC")], 3, min_count=2) == \
        b">0 LN:i:5 KC:i:8\nTCTTG\n"
    # no k-mer, no line
    assert out([("n", "ACNNGT")], 3) == b""
    # the complete set of canonical 3-mers: every side has four neighbours
    units = uc.unitigs(uc.table_of(CASES["all_3mers"][0], 3))
    assert len(units) == 32 and all(m == 1 for _, m, _ in units)
    assert [s for s, _, _ in units] == sorted(s for s, _, _ in units)


def _result(units, k):
    from kman_amd import engine

    off = np.cumsum([0] + [len(s) for s, _, _ in units]).astype(np.uint64)
    return engine.UnitigResult(np.frombuffer("".join(s for s, _, _ in units).encode(), dtype=np.uint8).copy(), off,
                               np.asarray([m for _, m, _ in units], dtype=np.uint32),
                               np.asarray([c for _, _, c in units], dtype=np.uint64), k)


def test_host_formatter_agrees_with_the_statement(monkeypatch, tmp_path):
    from ctypes import byref, c_size_t, c_void_p

    from kman_amd import _native as N
    from kman_amd import engine

    for name in ("two_cycles_and_paths", "all_5mers", "path_5000", "empty", "one_kmer"):
        records, k, min_count = CASES[name]
        units = uc.unitigs(uc.table_of(records, k, min_count))
        r = _result(units, k)
        assert r.n == len(units) and [r.seq(u) for u in range(r.n)] == [s for s, _, _ in units]
        assert engine.emit_unitigs(r) == uc.text(units)
        with open(tmp_path / "out.fa", "wb") as fh:
            assert engine.emit_unitigs(r, fh) is None
        assert (tmp_path / "out.fa").read_bytes() == uc.text(units)
    # slices of a few unitigs each: the IDs go on counting
    records, k, _ = CASES["all_5mers"]
    units = uc.unitigs(uc.table_of(records, k))
    monkeypatch.setattr(engine.unitig, "_UNITIG_SLICE", 37)
    assert engine.emit_unitigs(_result(units, k)) == uc.text(units)
    # counts up to 2^64 - 1, first_id, and the formatter's own refusals
    big = [("ACGTA", 1, (1 << 64) - 1), ("CC", 1, 0)]
    r = _result(big, 5)
    assert engine.emit_unitigs(r) == b">0 LN:i:5 KC:i:18446744073709551615\nACGTA\n>1 LN:i:2 KC:i:0\nCC\n"
    fn = N.lib().kman_format_unitigs
    used = c_size_t(0)
    args = (r.seqs.ctypes.data_as(c_void_p), r.off.ctypes.data_as(c_void_p), r.kc.ctypes.data_as(c_void_p), 2, 99)
    assert fn(*args, None, 0, byref(used), 2) == N.KMAN_ECAP and used.value == len(uc.text(big, 99))
    buf = (N.ctypes.c_char * used.value)()
    assert fn(*args, buf, used.value - 1, byref(used), 2) == N.KMAN_ECAP
    assert fn(*args, buf, used.value, byref(used), 2) == N.KMAN_OK and bytes(buf) == uc.text(big, 99)
    assert fn(None, None, None, 1, 0, None, 0, byref(used), 1) == N.KMAN_EINVAL
    bad = np.asarray([5, 2, 7], dtype=np.uint64)  # descending offsets
    assert fn(args[0], bad.ctypes.data_as(c_void_p), args[2], 2, 0, None, 0, byref(used), 1) == N.KMAN_EINVAL
    with pytest.raises(AssertionError):
        engine.emit_unitigs(engine.UnitigResult(r.seqs, r.off[:2], r.nodes, r.kc, 5))


def test_check_unitig_k():
    from kman_amd import engine

    for k in (3, 5, 21, 31):
        assert engine.check_unitig_k(k) == k
    for k, msg in ((4, "odd K"), (30, "odd K"), (33, "K <= 31"), (32, "K <= 31"), (1, "K >= 3"), (2, "K >= 3"),
                   (0, "K >= 3"), (-3, "K >= 3"), (True, "integer"), (21.0, "integer")):
        with pytest.raises(AssertionError, match=msg):
            engine.check_unitig_k(k)


def test_header_section_signatures_and_constants_agree():
    from kman_amd import _native as N

    with open(os.path.join(os.path.dirname(N.HERE), "include", "kman.h")) as fh:
        text = fh.read()
    assert re.search(r"#define\s+KMAN_ABI_VERSION\s+1\s", text)
    for name in ("KMAN_GRAPH_R", "KMAN_GRAPH_L", "KMAN_UNITIG_TILE"):
        m = re.search(r"#define\s+%s\s+(\d+)\s" % name, text)
        assert m and int(m.group(1)) == getattr(N, name), name
    assert (N.KMAN_GRAPH_R, N.KMAN_GRAPH_L) == (uc.R, uc.L)
    m = re.search(r"#define\s+KMAN_GRAPH_NONE\s+(0x[0-9A-Fa-f]+)u\s", text)
    assert m and int(m.group(1), 16) == N.KMAN_GRAPH_NONE == uc.NONE
    m = re.search(r"#define\s+KMAN_GRAPH_MAX_ROWS\s+\(1ull << (\d+)\)", text)
    assert m and 1 << int(m.group(1)) == N.KMAN_GRAPH_MAX_ROWS == 1 << 31
    for name, nargs in (("kman_graph_links", 7), ("kman_graph_rank", 8), ("kman_unitig_spell", 17),
                        ("kman_format_unitigs", 9)):
        assert name in N.header_symbols() and len(N.SIGNATURES[name][1]) == nargs, name
        decl = re.search(r"\bint %s\(([^;]*)\);" % name, text)
        assert decl and len(decl.group(1).split(",")) == nargs, name
        assert hasattr(N.lib(), name)
    assert sorted(N.SIGNATURES) == N.header_symbols()
    section = text[text.index("unitigs of a count table"):text.index("#define KMAN_GRAPH_R")]
    section = re.sub(r"\s*\n \*\s*", " ", section)  # the comment's lines joined
    for phrase in ("Not in the reference", "k is odd, 3 <= k <= 31", "deg(i, s) == 1", "j != i", "count twice",
                   "cut at side L of its smallest row", "the end row with the smaller index", "KMAN_EINVAL",
                   "nothing written", "nt == 0", "KMAN_ECAP", "never a wild address", "pointer doubling",
                   "ceil(log2(2 nt)) + 1", "No kernel loops over a unitig", '"graph_links"', '"graph_rank"',
                   '"unitig_spell"', "Synchronises", "modulo 2^64", ">ID LN:i:BASES KC:i:SUM"):
        assert phrase in section, phrase
    with open(os.path.join(N.HERE, "csrc", "Makefile")) as fh:
        assert "unitig.hip" in fh.read()
    with open(os.path.join(N.HERE, "csrc", "unitig.hip")) as fh:
        src = fh.read()
    for tag in ('"graph_links"', '"graph_rank"', '"unitig_spell"'):
        assert tag in src
    assert "asm" not in src and "table_rows<" in src and '#include "screen_lookup.h"' in src


# -------------------------------------------------------------------- the CLI


@pytest.fixture()
def inputs(tmp_path):
    fa = tmp_path / "a.fa"
    fa.write_bytes(b">s\nTTGCAACGTACGGATTACA\n")
    fq = tmp_path / "reads.fq"
    fq.write_bytes(b"@q\nACGTACGTTG\n+\nIIIIIIIIII\n")
    return fa, fq


def test_help_shows_every_option():
    from kman_amd.scripts.kmer import main

    run = CliRunner()
    text = run.invoke(main, ["unitigs", "--help"]).output
    for opt in ("INPUT", "OUTPUT", " K", "-f,", "--format", "-q,", "--min-qual", "--phred-offset", "-L,", "--min-count",
                "-U,", "--max-count", "--hpc", "--index-bits", "Not part of the reference", "LN:i:BASES", "KC:i:SUM",
                "GFA", "colours", "K > 31", "larger", "rank 0 alone"):
        assert opt in text, opt
    assert "--canonical" not in text and "READS" not in text
    assert "unitigs" in run.invoke(main, ["--help"]).output


def _refused_cases(tmp_path, inputs):
    fa, fq = inputs
    out = str(tmp_path / "out.fa")
    return {
        "k_even": ([str(fa), out, "20"], "odd K"),
        "k_4": ([str(fa), out, "4"], "odd K"),
        "k_33": ([str(fa), out, "33"], "K <= 31"),
        "k_32": ([str(fa), out, "32"], "K <= 31"),
        "k_1": ([str(fa), out, "1"], "K >= 3"),
        "k_2": ([str(fa), out, "2"], "K >= 3"),
        "output_gz": ([str(fa), out + ".gz", "21"], "ends in .gz"),
        "output_is_input": ([str(fa), str(fa), "21"], "same file"),
        "min_qual_without_fastq": ([str(fa), out, "21", "-q", "20"], "--min-qual needs fastq"),
        "min_above_max": ([str(fa), out, "21", "-L", "6", "-U", "5"], "--min-count 6 is greater than --max-count 5"),
        "index_bits_above_2k": ([str(fa), out, "3", "--index-bits", "7"], "--index-bits 7"),
    }


REFUSED = ["k_even", "k_4", "k_33", "k_32", "k_1", "k_2", "output_gz", "output_is_input", "min_qual_without_fastq",
           "min_above_max", "index_bits_above_2k"]


@pytest.mark.parametrize("case", REFUSED)
def test_refused_before_any_device_work_or_output(case, inputs, tmp_path, monkeypatch):
    from kman_amd import _native, engine
    from kman_amd.scripts.kmer import main

    def no_device(*a, **kw):
        raise RuntimeError("device work before the options were checked")

    monkeypatch.setattr(engine, "default_device", no_device)
    monkeypatch.setattr(engine, "Device", no_device)
    monkeypatch.setattr(_native, "lib", no_device)
    cases = _refused_cases(tmp_path, inputs)
    assert sorted(cases) == sorted(REFUSED)
    before = {p: p.read_bytes() for p in tmp_path.rglob("*") if p.is_file()}
    argv, msg = cases[case]
    r = CliRunner().invoke(main, ["unitigs"] + argv)
    assert isinstance(r.exception, AssertionError), (r.exception, r.output)
    assert msg in str(r.exception)
    assert {p: p.read_bytes() for p in tmp_path.rglob("*") if p.is_file()} == before  # nothing made or overwritten


@pytest.mark.parametrize("argv", [["21", "-L", "0"], ["21", "-q", "94"], ["five"], ["21", "--canonical"],
                                  ["21", "--index-bits", "25"]])
def test_usage_errors(argv, inputs, tmp_path):
    from kman_amd.scripts.kmer import main

    out = tmp_path / "out.fa"
    r = CliRunner().invoke(main, ["unitigs", str(inputs[0]), str(out)] + argv)
    assert r.exit_code == 2 and not out.exists()
    r = CliRunner().invoke(main, ["unitigs", "no/such/file.fa", str(out), "21"])
    assert r.exit_code == 2 and not out.exists()


def test_accepted_options_reach_the_device(inputs, tmp_path, monkeypatch):
    from kman_amd import engine
    from kman_amd.scripts.kmer import main

    class Reached(Exception):
        pass

    def device(*a, **kw):
        raise Reached()

    monkeypatch.setattr(engine, "default_device", device)
    for v in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "KMAN_DIST"):
        monkeypatch.delenv(v, raising=False)
    out = tmp_path / "out.fa"
    fa, fq = inputs
    for argv in ([str(fq), str(out), "5", "-q", "20"], [str(fa), str(out), "31", "-L", "2", "-U", "9"],
                 [str(fa), str(out), "3", "--index-bits", "6", "--hpc"], [str(fq), str(out), "21", "-f", "fastq"]):
        r = CliRunner().invoke(main, ["unitigs"] + argv)
        assert isinstance(r.exception, Reached), (r.exception, r.output)
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
    out = tmp_path / "out.fa"
    r = CliRunner().invoke(main, ["unitigs", str(inputs[0]), str(out), "21"])
    assert r.exception is None and r.exit_code == 0 and not out.exists()
    r = CliRunner().invoke(main, ["unitigs", str(inputs[0]), str(out), "20"])
    assert isinstance(r.exception, AssertionError)  # (refused on every rank)
