"""Read pairs without a GPU (`kmer screen` / `kmer classify --mate`,
`--interleaved`): the bindings and declarations of kman_zip_records, the pair
name rule on hand-worked cases, every refusal (raised before any device work or
output file), the formatter bytes of both TSV layouts, the views that cannot
free their codes, and the statement of the zip itself (tests/pair_cases.py) on
a hand-worked case."""

from __future__ import annotations

import os
import re

import numpy as np
import pytest
from click.testing import CliRunner

import pair_cases as pc


def _parsed(names, rec_seq=None, n_bases=0, codes=None):
    """A Parsed of these names on no device."""
    from kman_amd import engine

    names = [bytes(n) for n in names]
    off = np.zeros(len(names) + 1, np.uint64)
    off[1:] = np.cumsum([len(n) for n in names])
    blob = b"".join(names)
    R = len(names)
    rec_seq = np.arange(R, dtype=np.uint64) if rec_seq is None else np.asarray(rec_seq, np.uint64)
    return engine.Parsed(None, codes, n_bases, R, np.arange(R, dtype=np.uint64) * 10, rec_seq,
                         engine.BlobNames(blob, off), blob, off)


# ------------------------------------------------------------------ statement


def test_zip_statement_on_a_hand_worked_case():
    # mate 1: "AC", "", "G"; mate 2: "T", "TT", ""  (codes: A0 C1 G2 T3, +8 on a record's first base)
    c1, r1 = np.array([8, 1, 10], np.uint8), [0, 2, 2]
    c2, r2 = np.array([11, 11, 3], np.uint8), [0, 1, 3]
    codes, rec = pc.zip_codes(c1, r1, 3, c2, r2, 3)
    assert codes[:6].tolist() == [8, 1, 11, 11, 3, 10] and codes[6:].tolist() == [4] * 64
    assert rec.tolist() == [0, 2, 3, 3, 5, 6]  # an empty mate is an empty record
    codes, rec = pc.zip_codes(np.zeros(0, np.uint8), [], 0, np.zeros(0, np.uint8), [], 0)
    assert codes.tolist() == [4] * 64 and rec.tolist() == []
    assert pc.zip_records([("a", "AC"), ("b", "G")], [("a", "T"), ("b", "")]) == \
        [("a", "AC"), ("a", "T"), ("b", "G"), ("b", "")]


def test_pair_joint_statistics_are_sums_and_the_median_is_of_the_union():
    import median_cases as mc
    import screen_cases as sc

    k = 3
    table = {"ACG": 5, "CGT": 1, "TTT": 9}
    m1, m2 = [("p", "ACGT")], [("p", "TTTT")]
    st = pc.pair_stats(sc.stats(m1, k, table), sc.stats(m2, k, table))
    assert st.tolist() == [[4, 4, 5 + 1 + 9 + 9]]
    # mate 1's median is 1, mate 2's is 9, the pair's is the lower median of [1, 5, 9, 9]
    assert (mc.medians(m1, k, table), mc.medians(m2, k, table)) == ([1], [9])
    assert pc.pair_medians(m1, m2, k, table) == [5]
    # the last k - 1 bases of mate 1 and the first of mate 2 spell a table k-mer: nobody counts it
    table = {"GTT": 7}
    assert pc.pair_stats(sc.stats(m1, k, table), sc.stats(m2, k, table)).tolist() == [[4, 0, 0]]


def test_pair_selection_and_lines():
    st = np.array([[10, 5, 50], [10, 0, 0], [4, 4, 8]], np.uint64)
    med, s1, s2 = [3, 0, 2], [(0, 9), (0, 0), (1, 4)], [(2, 8), (0, 5), (0, 4)]
    assert pc.pair_keep(st, min_hits=1) == [True, False, True]
    assert pc.pair_keep(st, min_hits=1, invert=True) == [False, True, False]
    assert pc.pair_keep(st, med, min_median=3) == [True, False, False]
    assert pc.pair_keep(st, med, s1, s2, min_solid_len=4) == [True, False, False]  # both stretches
    assert pc.pair_keep(st, med, s1, s2, min_solid_len=3) == [True, False, True]
    assert pc.pair_lines(["a/1", "b/1", "c/1"], st, kept=[1, 0, 1]) == b"a/1\t10\t5\t50\nc/1\t4\t4\t8\n"
    assert pc.pair_lines(["a", "b", "c"], st, med, s1, s2, kept=[0, 0, 1]) == b"c\t4\t4\t8\t2\t1\t4\t0\t4\n"
    assert pc.pair_lines(["a"], st[:1], None, s1, s2) == b"a\t10\t5\t50\t0\t9\t2\t8\n"


# ---------------------------------------------------------------------- names


@pytest.mark.parametrize("i", range(len(pc.HAND_NAMES)))
def test_name_rule_on_hand_worked_cases(i):
    from kman_amd import engine

    a, b, ok = pc.HAND_NAMES[i]
    assert (pc.pair_key(a) == pc.pair_key(b)) == ok
    # the pair under test is the third of three
    p1, p2 = _parsed([b"x/1", b"y", a]), _parsed([b"x/2", b"y", b])
    if ok:
        engine.check_pair_names(p1, p2)
    else:
        with pytest.raises(AssertionError) as e:
            engine.check_pair_names(p1, p2)
        assert "pair 3" in str(e.value) and repr(a) in str(e.value) and repr(b) in str(e.value)


def test_name_check_names_the_first_bad_pair():
    from kman_amd import engine

    rng = np.random.default_rng(1)
    names = [b"read%d_%s" % (i, bytes(rng.integers(97, 123, int(rng.integers(0, 9))).tolist())) for i in range(500)]
    m1, m2 = [n + b"/1" for n in names], [n + b"/2" for n in names]
    engine.check_pair_names(_parsed(m1), _parsed(m2))
    engine.check_pair_names(_parsed(names), _parsed(m2))
    assert pc.first_name_mismatch(m1, m2) == -1
    for bad in ((317,), (499,), (0, 4), (120, 119)):
        other = list(m2)
        for j in bad:
            other[j] = other[j][:3] + b"X" + other[j][4:]  # (same length: a byte differs)
        other[min(bad)] = other[min(bad)] if len(bad) > 1 else other[min(bad)] + b"+"  # (or the length)
        first = pc.first_name_mismatch(m1, other)
        assert first == min(bad)
        with pytest.raises(AssertionError, match=r"pair %d:" % (first + 1)):
            engine.check_pair_names(_parsed(m1), _parsed(other))


def test_zip_pairs_refuses_before_any_device_work(monkeypatch):
    from kman_amd import _native, engine

    def no_device(*a, **kw):
        raise RuntimeError("device work before the inputs were checked")

    monkeypatch.setattr(_native, "lib", no_device)
    with pytest.raises(AssertionError) as e:
        engine.zip_pairs(_parsed([b"a", b"b", b"c"]), _parsed([b"a", b"b"]))
    assert "3 records" in str(e.value) and "2" in str(e.value)
    with pytest.raises(AssertionError, match="pair 2"):
        engine.zip_pairs(_parsed([b"a/1", b"b/1"]), _parsed([b"a/2", b"c/2"]))


# ---------------------------------------------------------------------- views


class _Owner:
    """A device buffer's double: counts what is freed."""

    def __init__(self):
        self.ptr, self.nbytes, self.dev, self.freed = 4096, 100, None, 0

    def free(self):
        self.freed += 1
        self.ptr = None


def test_pairs_of_refuses_an_odd_count_and_borrows_the_codes():
    from kman_amd import engine

    with pytest.raises(AssertionError, match="3 records"):
        engine.pairs_of(_parsed([b"a/1", b"a/2", b"b/1"]))
    with pytest.raises(AssertionError, match="pair 2"):
        engine.pairs_of(_parsed([b"a/1", b"a/2", b"b/1", b"c/2"]))
    owner = _Owner()
    p = _parsed([b"a/1", b"a/2", b"bb", b"bb", b"", b"/2"], rec_seq=[0, 5, 9, 9, 20, 21], n_bases=30, codes=owner)
    pv = engine.pairs_of(p)
    assert pv.n_records == 3 and pv.n_bases == 30 and pv.rec_seq.tolist() == [0, 9, 20]
    assert list(pv.names) == [b"a/1", b"bb", b""] and pv.names_blob == b"a/1bb" and pv.name_off.tolist() == [0, 3, 5, 5]
    assert pv.rec_hdr.tolist() == [0, 20, 40]
    assert pv.codes.ptr == 4096 and pv.codes.offset(8) == 4104
    pv.free()
    pv.free()
    assert owner.freed == 0 and pv.codes.ptr == 4096       # a view frees nothing, however often
    p.free()
    assert owner.freed == 1 and pv.codes.ptr is None       # and does not outlive the codes
    pv.free()
    assert owner.freed == 1
    assert engine.pairs_of(_parsed([])).n_records == 0


def test_pair_view_cannot_double_free():
    from kman_amd import engine

    owner, t1 = _Owner(), _Owner()
    p1 = _parsed([b"a/1", b"b/1"], rec_seq=[0, 4], n_bases=7, codes=_Owner())
    p1.text, p1.text_bytes = t1, 50
    p2 = _parsed([b"a/2", b"b/2"], rec_seq=[0, 3], n_bases=5, codes=_Owner())
    pz = engine.Parsed(None, owner, 12, 4, np.zeros(0, np.uint64), np.array([0, 4, 7, 10], np.uint64), [], b"",
                       np.zeros(1, np.uint64), mates=(p1, p2))
    pv = engine.pair_view(pz)
    assert pv.n_records == 2 and pv.rec_seq.tolist() == [0, 7] and list(pv.names) == [b"a/1", b"b/1"]
    assert pv.text is None and pv.mates is None and isinstance(pv.codes, engine.BorrowedBuffer)
    assert not hasattr(pv.codes, "__del__")
    pv.free()
    del pv
    assert owner.freed == 0
    pz.free()
    assert owner.freed == 1 and t1.freed == 1              # the result frees its sources' texts too
    with pytest.raises(AssertionError, match="zip_pairs"):
        engine.pair_view(p1)


def test_pair_min_span():
    from kman_amd import engine

    start, end = engine.pair_min_span((np.array([0, 2, 5, 0], np.uint64), np.array([9, 8, 5, 7], np.uint64)))
    assert start.tolist() == [0, 0] and end.tolist() == [6, 0]


# ------------------------------------------------------------------ formatter


def test_formatter_bytes_of_both_layouts():
    from kman_amd import engine

    pv = _parsed([b"a/1", b"", b"c c"])
    st = np.array([[10, 5, 50], [0, 0, 0], [4, 4, (1 << 64) - 1]], np.uint64)
    med = np.array([3, 0, 4294967294], np.uint32)
    span = (np.array([0, 2, 0, 0, 1, 0], np.uint64), np.array([9, 8, 0, 5, 4, 40], np.uint64))
    s1, s2 = [(0, 9), (0, 0), (1, 4)], [(2, 8), (0, 5), (0, 40)]
    names = ["a/1", "", "c c"]
    # the joint layout is the single reads' layout
    assert engine.emit_screen_pairs(pv, st, None) == pc.pair_lines(names, st)
    assert engine.emit_screen_pairs(pv, st, [1, 0, 1], median=med) == pc.pair_lines(names, st, med, kept=[1, 0, 1])
    # the solid layout: four span columns, after the median when there is one
    assert engine.emit_screen_pairs(pv, st, None, span=span) == pc.pair_lines(names, st, None, s1, s2)
    got = engine.emit_screen_pairs(pv, st, [0, 1, 1], median=med, span=span)
    assert got == pc.pair_lines(names, st, med, s1, s2, kept=[0, 1, 1])
    assert got == b"\t0\t0\t0\t0\t0\t0\t0\t5\nc c\t4\t4\t18446744073709551615\t4294967294\t1\t4\t0\t40\n"
    assert engine.emit_screen_pairs(pv, st, [0, 0, 0], span=span) == b""
    with pytest.raises(AssertionError):
        engine.emit_screen_pairs(pv, st, None, span=(span[0][:3], span[1][:3]))  # one row per mate is needed


# ------------------------------------------------------------------- bindings


def test_bindings_and_declarations():
    from kman_amd import _native as N

    with open(os.path.join(os.path.dirname(N.HERE), "include", "kman.h")) as fh:
        text = fh.read()
    for name in ("KMAN_ZIP_TILE", "KMAN_ZIP_SEG_CAP"):
        m = re.search(r"#define\s+%s\s+(\d+)\s" % name, text)
        assert m and int(m.group(1)) == getattr(N, name), name
    assert N.KMAN_ZIP_TILE % 4096 == 0 and N.KMAN_ZIP_SEG_CAP >= 2
    syms = N.header_symbols()
    for name, nargs in (("kman_zip_records", 10), ("kman_format_screen_pair", 12)):
        assert name in syms and name in N.SIGNATURES, name
        assert len(N.SIGNATURES[name][1]) == nargs, name
        decl = re.search(r"\bint %s\(([^;]*)\);" % name, text)
        assert decl and len(decl.group(1).split(",")) == nargs, name
        assert hasattr(N.lib(), name)
    assert sorted(N.SIGNATURES) == syms
    assert re.search(r"#define\s+KMAN_ABI_VERSION\s+1\s", text)
    with open(os.path.join(N.HERE, "csrc", "pair.hip")) as fh:
        src = fh.read()
    for line in ("constexpr uint32_t TILE = KMAN_ZIP_TILE", "constexpr int SEG_CAP = KMAN_ZIP_SEG_CAP"):
        assert line in src, line
    with open(os.path.join(N.HERE, "csrc", "Makefile")) as fh:
        assert "pair.hip" in fh.read()
    # a NULL context is refused on the host
    zip_ = N.lib().kman_zip_records
    assert zip_(None, None, 0, None, None, 0, None, 0, None, None) == N.KMAN_EINVAL


# ----------------------------------------------------------------------- CLI


@pytest.fixture()
def inputs(tmp_path):
    files = {
        "FA": (tmp_path / "reads.fa", b">r/1\nACGTACGTTGCAACGT\n"),
        "FA2": (tmp_path / "reads2.fa", b">r/2\nTTGCAACGTACGAAAA\n"),
        "FQ": (tmp_path / "reads.fq", b"@r/1\nACGTACGTTGCAACGT\n+\nIIIIIIIIIIIIIIII\n"),
        "FQ2": (tmp_path / "reads2.fq", b"@r/2\nTTGCAACGTACGAAAA\n+\nIIIIIIIIIIIIIIII\n"),
        "TABLE": (tmp_path / "genome.fa", b">s\nTTGCAACGTACG\n"),
    }
    for path, text in files.values():
        path.write_bytes(text)
    paths = {key: path for key, (path, _) in files.items()}
    for key in ("OUT", "BED", "R1", "R2", "R2.gz", "SUMMARY", "PREFIX"):
        paths[key] = tmp_path / ("out." + key.lower())
    return paths


def test_help_shows_the_pair_options():
    from kman_amd.scripts.kmer import main

    for cmd in ("screen", "classify"):
        text = CliRunner().invoke(main, [cmd, "--help"]).output
        for word in ("--mate", "-2", "READS2", "--interleaved", "kman_zip_records", "mates"):
            assert word in text, (cmd, word)
    assert "--reads-out2" in CliRunner().invoke(main, ["screen", "--help"]).output


# argv after `screen READS TABLE OUT 5`; READS is the fastq; capitals stand for paths
SCREEN_REFUSED = {
    "mate_and_interleaved": (["--mate", "FQ2", "--interleaved"], "exclude each other"),
    "bed": (["--mate", "FQ2", "--solid", "2", "--bed", "BED"], "--bed is not offered for read pairs"),
    "bed_interleaved": (["--interleaved", "--solid", "2", "--bed", "BED"], "--bed is not offered for read pairs"),
    "correct": (["--mate", "FQ2", "--solid", "2", "--correct"], "--correct is not offered for read pairs"),
    "correct_interleaved": (["--interleaved", "--solid", "2", "--correct"], "--correct is not offered for read pairs"),
    "mixed_formats": (["--mate", "FA2"], "mixed formats"),
    "reads_out2_without_mate": (["--reads-out", "R1", "--reads-out2", "R2"], "--reads-out2 needs --mate"),
    "reads_out2_interleaved": (["--interleaved", "--reads-out", "R1", "--reads-out2", "R2"],
                               "--reads-out2 needs --mate"),
    "reads_out_alone": (["--mate", "FQ2", "--reads-out", "R1"], "both or neither"),
    "reads_out2_alone": (["--mate", "FQ2", "--reads-out2", "R2"], "both or neither"),
    "reads_out2_gz": (["--mate", "FQ2", "--reads-out", "R1", "--reads-out2", "R2.gz"], ".gz"),
    "reads_out2_is_reads_out": (["--mate", "FQ2", "--reads-out", "R1", "--reads-out2", "R1"], "name the same file"),
    "reads_out2_is_output": (["--mate", "FQ2", "--reads-out", "R1", "--reads-out2", "OUT"], "name the same file"),
    "trim_without_solid": (["--mate", "FQ2", "--reads-out", "R1", "--reads-out2", "R2", "--trim"],
                           "--trim needs --solid"),
}


def _no_device(monkeypatch):
    from kman_amd import _native, engine

    def no_device(*a, **kw):
        raise RuntimeError("device work before the options were checked")

    monkeypatch.setattr(engine, "default_device", no_device)
    monkeypatch.setattr(engine, "Device", no_device)
    monkeypatch.setattr(_native, "lib", no_device)


@pytest.mark.parametrize("case", sorted(SCREEN_REFUSED))
def test_screen_refusals_before_any_device_work_or_output(case, inputs, monkeypatch):
    from kman_amd.scripts.kmer import main

    _no_device(monkeypatch)
    argv, msg = SCREEN_REFUSED[case]
    argv = [str(inputs.get(a, a)) for a in argv]
    r = CliRunner().invoke(main, ["screen", str(inputs["FQ"]), str(inputs["TABLE"]), str(inputs["OUT"]), "5"] + argv)
    assert isinstance(r.exception, AssertionError), (r.exception, r.output)
    assert msg in str(r.exception)
    assert not any(inputs[key].exists() for key in ("OUT", "BED", "R1", "R2", "R2.gz"))


CLASSIFY_REFUSED = {
    "mate_and_interleaved": (["--mate", "FQ2", "--interleaved"], "exclude each other"),
    "mixed_formats": (["--mate", "FA2"], "mixed formats"),
    "prefix_file_is_output": (["--mate", "FQ2", "--reads-out-prefix", "PREFIX"], "name the same file"),
}


@pytest.mark.parametrize("case", sorted(CLASSIFY_REFUSED))
def test_classify_refusals_before_any_device_work_or_output(case, inputs, monkeypatch):
    from kman_amd.scripts.kmer import main

    _no_device(monkeypatch)
    argv, msg = CLASSIFY_REFUSED[case]
    argv = [str(inputs.get(a, a)) for a in argv]
    out = str(inputs["PREFIX"]) + ".genome.2.fq" if case == "prefix_file_is_output" else str(inputs["OUT"])
    r = CliRunner().invoke(main, ["classify", str(inputs["FQ"]), out, "5", "--ref", str(inputs["TABLE"])] + argv)
    assert isinstance(r.exception, AssertionError), (r.exception, r.output)
    assert msg in str(r.exception)
    assert not os.path.exists(out)


def test_classify_pair_outputs():
    from kman_amd import engine
    from kman_amd.scripts.kmer import _classify_pair_outputs

    assert _classify_pair_outputs(None, ["a"], "fq") == []
    assert _classify_pair_outputs("p", ["hs", "mm"], "fq") == [
        (0, "p.hs.1.fq", "p.hs.2.fq"), (1, "p.mm.1.fq", "p.mm.2.fq"),
        (engine.AMBIGUOUS, "p.ambiguous.1.fq", "p.ambiguous.2.fq"),
        (engine.UNASSIGNED, "p.unassigned.1.fq", "p.unassigned.2.fq")]
    assert _classify_pair_outputs("p", ["x"], "fa")[0] == (0, "p.x.1.fa", "p.x.2.fa")


def test_check_screen_options_keeps_its_old_callers():
    from kman_amd.scripts.kmer import _check_screen_options

    _check_screen_options(5, 0, [False, False], 1, None, 0, 0.0, None)
    _check_screen_options(5, 0, [True, False], 1, None, 0, 0.0, None, solid=2, reads_out="a.fq", trim=True,
                          output_path="a.tsv", bed_path="a.bed")
    _check_screen_options(5, 0, [True, False], 1, None, 0, 0.0, None, solid=2, reads_out="a.fq", reads_out2="b.fq",
                          trim=True, output_path="a.tsv", mate_path="m.fq", fastq_mate=True)
    _check_screen_options(5, 0, [True, False], 1, None, 0, 0.0, None, reads_out="a.fq", output_path="a.tsv",
                          interleaved=True)


def test_a_run_without_the_options_makes_todays_calls(inputs, monkeypatch):
    """Without --mate / --interleaved the reads are parsed by the one call the
    command made before, and no pair function is reached."""
    from kman_amd import engine
    from kman_amd.scripts import kmer

    class Reached(Exception):
        pass

    class _P:
        def free(self):
            pass

    calls = []

    def parse_file(dev, path, *a, **kw):
        calls.append((os.path.basename(path), kw))
        return _P()

    def reached(*a, **kw):
        raise Reached()

    def never(*a, **kw):
        raise AssertionError("a pair function in a run without pairs")

    for v in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "KMAN_DIST"):
        monkeypatch.delenv(v, raising=False)
    monkeypatch.setattr(engine, "default_device", lambda *a, **kw: None)
    monkeypatch.setattr(engine, "parse_file", parse_file)
    monkeypatch.setattr(engine, "check_empty_names", lambda *a, **kw: None)
    monkeypatch.setattr(engine, "join_groups", lambda *a, **kw: object())
    monkeypatch.setattr(engine, "free_result", lambda *a, **kw: None)
    monkeypatch.setattr(engine, "screen", reached)
    for name in ("zip_pairs", "pair_view", "pairs_of", "screen_pairs"):
        monkeypatch.setattr(engine, name, never)
    r = CliRunner().invoke(kmer.main, ["screen", str(inputs["FQ"]), str(inputs["TABLE"]), str(inputs["OUT"]), "5"])
    assert isinstance(r.exception, Reached), (r.exception, r.output)
    assert calls == [("genome.fa", {}), ("reads.fq", {})]
