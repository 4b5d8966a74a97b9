"""`kmer screen --reads-out` / `--trim` without a GPU: the plain-Python
statement of kman_cut_records' bytes (tests/reads_cases.py) pinned to
hand-written cases and to the FASTQ rules of fastq_cases, the CLI's new
refusals (raised before any device work or output file), the plan call and
the ABI's constants."""

from __future__ import annotations

import ctypes
import os
import re
from ctypes import byref, c_size_t, c_uint64

import numpy as np
import pytest
from click.testing import CliRunner

import fastq_cases as fq
import reads_cases as rcs


# ------------------------------------------------------------------ statement


@pytest.mark.parametrize("i", range(len(rcs.HAND_TRIM)))
def test_trimmed_record_on_hand_written_cases(i):
    rec, s, e, want = rcs.HAND_TRIM[i]
    assert rcs.trimmed_record(rec, s, e) == want


def test_whole_records_on_hand_written_cases():
    text = b"junk\n@a\r\nAC\r\n+\r\n!!\r\n@b x\rG T\r+b\r#$%\r@c\nacgt\n+\nIIII"  # CRLF, lone CR, no final newline
    off = [text.index(b"@a"), text.index(b"@b"), text.index(b"@c"), len(text)]
    assert off[:3] == [5, 20, 36]
    assert rcs.cut_whole(text, off) == text[5:]                      # bytes before the first record are never written
    assert rcs.cut_whole(text, off, [0, 1, 0]) == b"@b x\rG T\r+b\r#$%\r"
    assert rcs.cut_whole(text, off, [1, 0, 1]) == b"@a\r\nAC\r\n+\r\n!!\r\n@c\nacgt\n+\nIIII"
    assert rcs.cut_whole(text, off, [0, 0, 0]) == b""
    # trailing empty lines stay with the last record; lower case and blanks stay as they are
    assert rcs.cut_whole(b"@r\nac gt\n+\nIIIII\n\n\r\n", [0, 20]) == b"@r\nac gt\n+\nIIIII\n\n\r\n"
    # clamped offsets, a descending pair
    assert rcs.cut_whole(b"0123456789", [2, 5, 3, 8, 99, 4]) == b"234" + b"" + b"34567" + b"89" + b""
    # the three records trimmed, terminators normalised
    assert rcs.cut_trimmed(text, off, [0, 1, 1], [1, 2, 9]) == b"@a\nA\n+\n!\n@b x\nT\n+b\n%\n@c\ncgt\n+\nIII\n"


def test_fastq_offsets_are_the_parser_rules_record_starts():
    for nl in (b"\n", b"\r\n", b"\r"):
        text = fq.mixed_reads(seed=3, n_records=50, nl=nl)
        lines = fq.fastq_lines(text)
        off = rcs.fastq_offsets(text)
        assert len(off) - 1 == len(lines) // 4
        assert all(text[o:o + 1] == b"@" for o in off[:-1]) and off[0] == 0
        assert rcs.cut_whole(text, off) == text
        for r, rec in enumerate(rcs.records_of(text, off)):
            assert rcs.record_lines(rec) == lines[4 * r:4 * r + 4]


def test_cols_are_the_bytes_that_get_a_code():
    """The kept columns of every record's sequence line are as many as the
    record's bases in the FASTA of the same records, and spell them."""
    rng = np.random.default_rng(5)
    recs = []
    for i in range(40):
        n = int(rng.integers(0, 80))
        seq = bytearray(fq.seq_of(rng, n))
        for at in rng.integers(0, max(n, 1), n // 6).tolist():
            if n:
                seq[at] = 0x20
        seq = bytes(seq) + (b"", b" ", b"\t ", b" \x0b\x0c", b"\x1c\x1f ")[i % 5]
        recs.append(fq.record(b"r%d" % i, seq, fq.qual_of(rng, len(seq)), nl=(b"\n", b"\r\n")[i % 2]))
    text = b"".join(recs)
    fasta = fq.fastq_to_fasta(text).split(b"\n")[:-1]
    assert len(fasta) == 2 * len(recs)
    for r, rec in enumerate(rcs.records_of(text, rcs.fastq_offsets(text))):
        l2 = rcs.record_lines(rec)[1]
        # the cleaning of a FASTA sequence line (str.rstrip, as the reference's text-mode reader strips)
        bases = fasta[2 * r + 1].decode("latin-1").rstrip().replace(" ", "").replace("\r", "").encode("latin-1")
        cols = rcs.cols_of(l2)
        assert len(cols) == len(bases) and bytes(l2[c] for c in cols) == bases
        if cols:
            whole = rcs.trimmed_record(rec, 0, len(cols)).split(b"\n")
            assert whole[1] == l2[cols[0]:cols[-1] + 1] and len(whole[3]) == len(whole[1])


def test_host_loop_of_the_engine_is_the_statement():
    from kman_amd import engine

    text = fq.mixed_reads(seed=8, n_records=60, nl=b"\r\n") + b"".join(c[0] for c in rcs.HAND_TRIM[:4])
    off = rcs.fastq_offsets(text)
    R = len(off) - 1
    rng = np.random.default_rng(9)
    start = rng.integers(0, 30, R)
    end = start + rng.integers(0, 60, R)
    keep = rng.integers(0, 2, R)
    assert engine._cut_host(text, off, keep, None, False) == rcs.cut_whole(text, off, keep)
    assert engine._cut_host(text, off, None, (start, end), True) == rcs.cut_trimmed(text, off, start, end)
    assert engine._cut_host(text, off, keep, (start, end), True) == rcs.cut_trimmed(text, off, start, end, keep)


def test_cut_slices():
    from kman_amd import engine

    bound = np.array([10, 0, 30, 500, 5, 5, 0, 0, 90, 10], np.int64)
    sl = engine._cut_slices(bound, 100)
    assert [(i0, m) for i0, m, _ in sl] == [(0, 3), (3, 1), (4, 5), (9, 1)]  # the large record in a slice of its own
    assert [b for _, _, b in sl] == [40, 500, 100, 10]
    assert sum(m for _, m, _ in sl) == len(bound) and sum(b for _, _, b in sl) == int(bound.sum())
    assert engine._cut_slices(np.zeros(5, np.int64), 100) == [(0, 5, 0)]


# ----------------------------------------------------------------------- CLI


@pytest.fixture()
def inputs(tmp_path):
    fa = tmp_path / "reads.fa"
    fa.write_bytes(b">r\nACGTACGTTGCAACGT\n")
    fb = tmp_path / "genome.fa"
    fb.write_bytes(b">s\nTTGCAACGTACG\n")
    fqp = tmp_path / "reads.fq"
    fqp.write_bytes(b"@r\nACGTACGTTGCAACGT\n+\nIIIIIIIIIIIIIIII\n")
    return fa, fb, fqp


def test_help_shows_the_reads_options():
    from kman_amd.scripts.kmer import main

    text = CliRunner().invoke(main, ["screen", "--help"]).output
    for opt in ("--reads-out", "--trim", "FILE", "uncompressed", "kman_cut_records"):
        assert opt in text, opt


# argv after K; READS is the fasta unless "FQ" is named; OUT, BED and READS_OUT stand for paths
REFUSED = {
    "trim_without_solid": (["FQ", "--trim", "--reads-out", "READS_OUT"], "--trim needs --solid"),
    "trim_without_reads_out": (["FQ", "--trim", "--solid", "2"], "--trim needs --reads-out"),
    "trim_with_fasta_reads": (["--trim", "--solid", "2", "--reads-out", "READS_OUT"], "--trim needs fastq READS"),
    "reads_out_gz": (["--reads-out", "READS_OUT.gz"], ".gz"),
    "reads_out_is_output": (["--reads-out", "OUT"], "name the same file"),
    "reads_out_is_bed": (["--solid", "2", "--bed", "BED", "--reads-out", "BED"], "name the same file"),
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
    paths = {"OUT": tmp_path / "out.tsv", "BED": tmp_path / "out.bed", "READS_OUT": tmp_path / "out.fq",
             "READS_OUT.gz": tmp_path / "out.fq.gz"}
    reads = inputs[2] if "FQ" in argv else inputs[0]
    argv = [str(paths.get(a, a)) for a in argv if a != "FQ"]
    r = CliRunner().invoke(main, ["screen", str(reads), str(inputs[1]), str(paths["OUT"]), "5"] + argv)
    assert isinstance(r.exception, AssertionError), (r.exception, r.output)
    assert msg in str(r.exception)
    assert not any(p.exists() for p in paths.values())


def test_check_screen_options_keeps_its_old_callers():
    from kman_amd.scripts.kmer import _check_screen_options

    _check_screen_options(5, 0, [False, False], 1, None, 0, 0.0, None)
    _check_screen_options(5, 0, [False, False], 1, None, 0, 0.0, None, None, None, 2, 10, "x.bed")
    _check_screen_options(5, 0, [True, False], 1, None, 0, 0.0, None, solid=2, reads_out="a.fq", trim=True,
                          output_path="a.tsv", bed_path="a.bed")
    with pytest.raises(AssertionError, match="same file"):
        _check_screen_options(5, 0, [True, False], 1, None, 0, 0.0, None, reads_out="./a.tsv", output_path="a.tsv")


@pytest.mark.parametrize("argv, keep_text", [([], False), (["--reads-out", "READS_OUT"], True)])
def test_text_is_kept_only_with_reads_out(argv, keep_text, inputs, tmp_path, monkeypatch):
    """READS is parsed with keep_text=True only under --reads-out; without it the call is today's."""
    from kman_amd import engine
    from kman_amd.scripts import kmer

    class Reached(Exception):
        pass

    class _Parsed:
        def free(self):
            pass

    calls = []

    def parse_file(dev, path, *a, **kw):
        calls.append((os.path.basename(path), kw))
        return _Parsed()

    def reached(*a, **kw):
        raise Reached()

    for v in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "KMAN_DIST"):
        monkeypatch.delenv(v, raising=False)
    monkeypatch.setattr(engine, "default_device", lambda *a, **kw: None)
    monkeypatch.setattr(engine, "parse_file", parse_file)
    monkeypatch.setattr(engine, "check_empty_names", lambda *a, **kw: None)
    monkeypatch.setattr(engine, "join_groups", lambda *a, **kw: object())
    monkeypatch.setattr(engine, "free_result", lambda *a, **kw: None)
    monkeypatch.setattr(engine, "screen", reached)
    argv = [str(tmp_path / "out.fq") if a == "READS_OUT" else a for a in argv]
    r = CliRunner().invoke(kmer.main, ["screen", str(inputs[2]), str(inputs[1]), str(tmp_path / "out.tsv"), "5"] + argv)
    assert isinstance(r.exception, Reached), (r.exception, r.output)
    assert calls == [("genome.fa", {}), ("reads.fq", {"keep_text": True} if keep_text else {})]


# ------------------------------------------------------------ plan, constants


def test_plan_call_and_null_context():
    from kman_amd import _native as N

    L = ctypes.CDLL(N.LIB_PATH)  # (host only: no device is asked for)
    fn = L.kman_cut_records_plan
    fn.restype, fn.argtypes = N.SIGNATURES["kman_cut_records_plan"]

    def plan(nr, flags):
        out = c_uint64(123)
        rc = fn(nr, flags, byref(out))
        return rc, out.value

    assert plan(0, 0) == (N.KMAN_OK, 16)
    for n in (1, 2, 1000, 12345):
        rc, whole = plan(n, 0)
        rc2, trim = plan(n, N.KMAN_CUT_TRIM)
        assert rc == rc2 == N.KMAN_OK and whole % 16 == 0 and trim % 16 == 0
        assert 16 * n + 8 <= whole <= 16 * n + 16 and 64 * n + 8 <= trim <= 64 * n + 16
    assert fn(1, 0, None) == N.KMAN_EINVAL
    assert plan(1, 2) == (N.KMAN_EINVAL, 0) and plan(1, N.KMAN_CUT_TRIM | 8) == (N.KMAN_EINVAL, 0)
    assert plan((1 << 31) + 1, 0) == (N.KMAN_EINVAL, 0) and plan(1 << 31, 0)[0] == N.KMAN_OK
    cut = L.kman_cut_records
    cut.restype, cut.argtypes = N.SIGNATURES["kman_cut_records"]
    used = c_size_t(5)
    assert cut(None, None, 0, None, 0, None, None, None, 0, None, 0, None, 0, byref(used)) == N.KMAN_EINVAL


def test_header_signatures_and_constants_agree():
    from kman_amd import _native as N

    with open(os.path.join(os.path.dirname(N.HERE), "include", "kman.h")) as fh:
        text = fh.read()
    for name in ("KMAN_CUT_TILE", "KMAN_CUT_SEG_CAP"):
        m = re.search(r"#define\s+%s\s+(\d+)\s" % name, text)
        assert m and int(m.group(1)) == getattr(N, name), name
    m = re.search(r"#define\s+KMAN_CUT_TRIM\s+(\d+)u\s", text)
    assert m and int(m.group(1)) == N.KMAN_CUT_TRIM
    assert N.KMAN_CUT_TILE % 4096 == 0
    syms = N.header_symbols()
    for name, nargs in (("kman_cut_records_plan", 3), ("kman_cut_records", 14)):
        assert name in syms and name in N.SIGNATURES, name
        assert len(N.SIGNATURES[name][1]) == nargs, name
        decl = re.search(r"\bint %s\(([^;]*)\);" % name, text)
        assert decl and len(decl.group(1).split(",")) == nargs, name
    assert sorted(N.SIGNATURES) == syms
    assert re.search(r"#define\s+KMAN_ABI_VERSION\s+1\s", text)
    with open(os.path.join(N.HERE, "csrc", "cut.hip")) as fh:
        src = fh.read()
    for line in ("constexpr uint32_t TILE = KMAN_CUT_TILE", "constexpr int SEG_CAP = KMAN_CUT_SEG_CAP"):
        assert line in src, line
    with open(os.path.join(N.HERE, "csrc", "Makefile")) as fh:
        assert "cut.hip" in fh.read()
