"""`kmer classify` without a GPU: the command's options, every refusal raised
before any device work or output file, the ABI's constants and signatures,
the host formatter kman_format_classify, engine.classify_assign, the label
rule, and the plain-Python statement (tests/classify_cases.py) pinned to a
hand-written three-reference example."""

from __future__ import annotations

import ctypes
import gzip
import os
import re
from ctypes import byref, c_size_t, c_void_p

import numpy as np
import pytest
from click.testing import CliRunner

import classify_cases as cc
import screen_cases as sc


@pytest.fixture()
def inputs(tmp_path):
    fa = tmp_path / "reads.fa"
    fa.write_bytes(b">r\nACGTACGTTGCAACGT\n")
    a = tmp_path / "a.fa"
    a.write_bytes(b">s\nTTGCAACGTACG\n")
    b = tmp_path / "b.fa"
    b.write_bytes(b">t\nGGGGGGCCCCACGT\n")
    fq = tmp_path / "reads.fq"
    fq.write_bytes(b"@q\nACGTACGTTG\n+\nIIIIIIIIII\n")
    return fa, a, b, fq


def test_help_shows_every_option():
    from kman_amd.scripts.kmer import main

    run = CliRunner()
    text = run.invoke(main, ["classify", "--help"]).output
    for opt in ("READS", "OUTPUT", " K", "--ref", "--canonical", "-f,", "--format", "-q,", "--min-qual",
                "--phred-offset", "-L,", "--min-count", "-U,", "--max-count", "--specific", "--min-hits",
                "--min-frac", "--min-margin", "--hits", "--summary", "--reads-out-prefix", "--index-bits",
                "Not part of the reference"):
        assert opt in text, opt
    assert "TABLE_INPUT" not in text and "--invert" not in text
    assert "classify" in run.invoke(main, ["--help"]).output


def _refused_cases(tmp_path, inputs):
    """name -> (argv after READS, the message, paths that must not exist)."""
    fa, a, b, fq = inputs
    out = tmp_path / "out.tsv"
    d = tmp_path / "d"
    d.mkdir()
    (d / "a.fa").write_bytes(b">u\nACGTACGT\n")
    with gzip.open(d / "b.fasta.gz", "wb") as fh:
        fh.write(b">u\nACGTACGT\n")
    many = []
    for i in range(65):
        path = d / ("m%d.fa" % i)
        path.write_bytes(b">u\nACGTACGT\n")
        many += ["--ref", str(path)]
    odd = {}
    for name in ("-.fa", "?.fa", "ambiguous.fa.gz", "unassigned.fq", "with\ttab.fa"):
        path = d / name
        if name.endswith(".gz"):
            with gzip.open(path, "wb") as fh:
                fh.write(b">u\nACGTACGT\n")
        elif name.endswith(".fq"):
            path.write_bytes(b"@u\nACGTACGT\n+\nIIIIIIII\n")
        else:
            path.write_bytes(b">u\nACGTACGT\n")
        odd[name] = str(path)
    ra, rb = ["--ref", str(a)], ["--ref", str(b)]
    pre = tmp_path / "cut"
    return out, {
        "no_ref": ([str(out), "5"], "1 to 64 --ref"),
        "65_refs": ([str(out), "5"] + many, "1 to 64 --ref"),
        "equal_labels": ([str(out), "5"] + ra + ["--ref", str(d / "a.fa")], "label 'a'"),
        "equal_labels_gz": ([str(out), "5"] + rb + ["--ref", str(d / "b.fasta.gz")], "label 'b'"),
        "label_dash": ([str(out), "5"] + ra + ["--ref", odd["-.fa"]], "reserved"),
        "label_question": ([str(out), "5", "--ref", odd["?.fa"]], "reserved"),
        "label_ambiguous": ([str(out), "5"] + ra + ["--ref", odd["ambiguous.fa.gz"]], "reserved"),
        "label_unassigned": ([str(out), "5", "--ref", odd["unassigned.fq"]], "reserved"),
        "label_tab": ([str(out), "5"] + ra + ["--ref", odd["with\ttab.fa"]], "tab"),
        "k_1": ([str(out), "1"] + ra, "k must be >= 1"),
        "k_33": ([str(out), "33"] + ra, "K <= 32"),
        "k_40": ([str(out), "40"] + ra + rb, "stated limit"),
        "min_qual_without_fastq": ([str(out), "5", "-q", "20"] + ra + rb, "--min-qual"),
        "min_above_max": ([str(out), "5", "-L", "6", "-U", "5"] + ra, "--min-count 6 is greater than --max-count 5"),
        "min_margin_0": ([str(out), "5", "--min-margin", "0"] + ra, "--min-margin"),
        "min_margin_negative": ([str(out), "5", "--min-margin=-2"] + ra, "--min-margin"),
        "min_frac_above_1": ([str(out), "5", "--min-frac", "1.5"] + ra, "--min-frac"),
        "min_frac_nan": ([str(out), "5", "--min-frac", "nan"] + ra, "--min-frac"),
        "min_hits_negative": ([str(out), "5", "--min-hits=-1"] + ra, "--min-hits"),
        "index_bits_above_2k": ([str(out), "5", "--index-bits", "11"] + ra, "--index-bits"),
        "summary_is_output": ([str(out), "5", "--summary", str(out)] + ra, "same file"),
        "prefix_file_is_output": ([str(pre) + ".a.fa", "5", "--reads-out-prefix", str(pre)] + ra + rb, "same file"),
        "prefix_unassigned_is_output": ([str(pre) + ".unassigned.fa", "5", "--reads-out-prefix", str(pre)] + ra,
                                        "same file"),
        "prefix_file_is_summary": ([str(out), "5", "--reads-out-prefix", str(pre), "--summary",
                                    str(pre) + ".ambiguous.fa"] + ra, "same file"),
    }


REFUSED = ["no_ref", "65_refs", "equal_labels", "equal_labels_gz", "label_dash", "label_question", "label_ambiguous",
           "label_unassigned", "label_tab", "k_1", "k_33", "k_40", "min_qual_without_fastq", "min_above_max",
           "min_margin_0", "min_margin_negative", "min_frac_above_1", "min_frac_nan", "min_hits_negative",
           "index_bits_above_2k", "summary_is_output", "prefix_file_is_output", "prefix_unassigned_is_output",
           "prefix_file_is_summary"]


@pytest.mark.parametrize("case", REFUSED)
def test_refused_before_any_device_work_or_output(case, inputs, tmp_path, monkeypatch):
    from kman_amd import _native, engine
    from kman_amd.scripts.kmer import main

    def no_device(*a, **kw):
        raise RuntimeError("device work before the options were checked")

    monkeypatch.setattr(engine, "default_device", no_device)
    monkeypatch.setattr(engine, "Device", no_device)
    monkeypatch.setattr(_native, "lib", no_device)
    out, cases = _refused_cases(tmp_path, inputs)
    assert sorted(cases) == sorted(REFUSED)
    before = {p for p in tmp_path.rglob("*")}
    argv, msg = cases[case]
    r = CliRunner().invoke(main, ["classify", str(inputs[0])] + argv)
    assert isinstance(r.exception, AssertionError), (r.exception, r.output)
    assert msg in str(r.exception)
    assert {p for p in tmp_path.rglob("*")} == before  # no output, summary or cut file was made


@pytest.mark.parametrize("argv", [[], ["5", "--index-bits", "0"], ["5", "-L", "0"], ["5", "--min-frac", "half"],
                                  ["5", "-v"], ["5", "--ref", "no/such/file.fa"]])
def test_usage_errors(argv, inputs, tmp_path):
    from kman_amd.scripts.kmer import main

    out = tmp_path / "out.tsv"
    r = CliRunner().invoke(main, ["classify", str(inputs[0]), str(out)] + argv + ["--ref", str(inputs[1])])
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
    fa, a, b, fq = inputs
    for reads, ref in ((fq, a), (fa, fq)):
        r = CliRunner().invoke(main, ["classify", str(reads), str(out), "5", "-q", "20", "--ref", str(ref), "--ref",
                                      str(b)])
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
    out = tmp_path / "out.tsv"
    r = CliRunner().invoke(main, ["classify", str(inputs[0]), str(out), "5", "--ref", str(inputs[1])])
    assert r.exception is None and r.exit_code == 0 and not out.exists()
    r = CliRunner().invoke(main, ["classify", str(inputs[0]), str(out), "40", "--ref", str(inputs[1])])
    assert isinstance(r.exception, AssertionError)  # (refused on every rank)


def test_header_signatures_and_constants_agree():
    from kman_amd import _native as N

    with open(os.path.join(os.path.dirname(N.HERE), "include", "kman.h")) as fh:
        text = fh.read()
    for name in ("KMAN_CLASSIFY_MAX_COLORS", "KMAN_CLASSIFY_SPECIFIC", "KMAN_CLASSIFY_NONE"):
        m = re.search(r"#define\s+%s\s+(0x[0-9A-Fa-f]+|\d+)u?\s" % name, text)
        assert m and int(m.group(1), 0) == getattr(N, name), name
    assert N.KMAN_CLASSIFY_MAX_COLORS == 64 and N.KMAN_CLASSIFY_NONE == 0xFFFFFFFF
    # a flag bit of its own beside KMAN_CANONICAL
    assert N.KMAN_CLASSIFY_SPECIFIC & (N.KMAN_CLASSIFY_SPECIFIC - 1) == 0
    assert N.KMAN_CLASSIFY_SPECIFIC != N.KMAN_CANONICAL
    syms = N.header_symbols()
    for name, nargs in (("kman_classify_records", 14), ("kman_classify_pick", 5), ("kman_format_classify", 16)):
        assert name in syms and name in N.SIGNATURES, name
        assert len(N.SIGNATURES[name][1]) == nargs, name
        decl = re.search(r"\bint %s\(([^;]*)\);" % name, text)
        assert decl and len(decl.group(1).split(",")) == nargs, name
    assert sorted(N.SIGNATURES) == syms
    assert re.search(r"#define\s+KMAN_ABI_VERSION\s+1\s", text)
    with open(os.path.join(N.HERE, "csrc", "classify.hip")) as fh:
        src = fh.read()
    assert "static_assert(CTILE == KMAN_SCREEN_TILE" in src and "CCAP = KMAN_SCREEN_REC_CAP" in src
    assert "table_lookup<CEI, uint64_t>" in src
    with open(os.path.join(N.HERE, "csrc", "Makefile")) as fh:
        assert "classify.hip" in fh.read()


def test_labels():
    from kman_amd.scripts.kmer import ref_label

    want = {"a.fa": "a", "dir/a.fa.gz": "a", "/x/y/b.fastq.gz": "b", "noext": "noext", "noext.gz": "noext",
            "two.dots.fasta": "two.dots", "sample.1.fq.gz": "sample.1"}
    for path, label in want.items():
        assert ref_label(path) == label == cc.label_of(path), path


# ------------------------------------------------------------ host formatter


def _format_classify(windows, assign, hits, second, names, labels, planes=None, keep=None, cap=None, threads=3):
    """(return code, used, text) of one kman_format_classify call."""
    from kman_amd import _native as N

    L = ctypes.CDLL(N.LIB_PATH)  # (the formatter is host code: no device is asked for)
    fn = L.kman_format_classify
    fn.restype, fn.argtypes = N.SIGNATURES["kman_format_classify"]
    w, h, s = (np.ascontiguousarray(a, dtype=np.uint32) for a in (windows, hits, second))
    a = np.ascontiguousarray(assign, dtype=np.int32)
    n = len(w)

    def blob_of(items):
        off = np.zeros(len(items) + 1, dtype=np.uint64)
        off[1:] = np.cumsum([len(x) for x in items])
        return b"".join(items), off

    nb, noff = blob_of(names)
    lb, loff = blob_of(labels)
    pp = None
    if planes is not None:
        planes = np.ascontiguousarray(planes, dtype=np.uint32)
        assert planes.shape == (len(labels), n)
        pp = planes.ctypes.data_as(c_void_p)
    kp = None
    if keep is not None:
        keep = np.asarray(keep, dtype=np.uint8)
        kp = keep.ctypes.data_as(c_void_p)
    used = c_size_t(0)
    buf = ctypes.create_string_buffer(max(1, cap)) if cap is not None else None
    rc = fn(w.ctypes.data_as(c_void_p), a.ctypes.data_as(c_void_p), h.ctypes.data_as(c_void_p),
            s.ctypes.data_as(c_void_p), pp, len(labels), n, kp, lb, loff.ctypes.data_as(c_void_p), nb,
            noff.ctypes.data_as(c_void_p), buf, cap or 0, byref(used), threads)
    return rc, used.value, (buf.raw[:used.value] if buf is not None and rc == 0 else None)


def test_format_classify():
    from kman_amd import _native as N

    top = (1 << 32) - 1
    windows = [136, 0, 5, top, 10, 7]
    assign = [0, -1, 2, 1, -2, 0]
    hits = [100, 0, 5, top, 3, 7]
    second = [0, 0, 4, top - 1, 3, 6]
    names = [b"read1", b"", b"with\ttab", b"r/1", b"x" * 300, b"last"]
    labels = [b"human", b"m", b"a.long.label-with_things"]
    planes = np.asarray([[100, 0, 4, 0, 3, 7], [0, 0, 1, top, 3, 6], [0, 0, 5, top - 1, 1, 0]], dtype=np.uint32)
    recs = [(n.decode(), "") for n in names]
    ltxt = [x.decode() for x in labels]
    want = cc.lines(recs, ltxt, windows, assign, hits, second)
    assert want.startswith(b"read1\t136\thuman\t100\t0\n\t0\t-\t0\t0\n") and b"\t?\t3\t3\n" in want
    rc, used, _ = _format_classify(windows, assign, hits, second, names, labels)  # sizing call: no buffer
    assert (rc, used) == (N.KMAN_ECAP, len(want))
    rc, used, text = _format_classify(windows, assign, hits, second, names, labels, cap=len(want))
    assert (rc, used, text) == (N.KMAN_OK, len(want), want)
    rc, used, _ = _format_classify(windows, assign, hits, second, names, labels, cap=len(want) - 1)
    assert (rc, used) == (N.KMAN_ECAP, len(want))  # one byte short: refused, the size reported
    wantp = cc.lines(recs, ltxt, windows, assign, hits, second, planes)
    assert wantp.endswith(b"last\t7\thuman\t7\t6\t7\t6\t0\n")
    rc, used, text = _format_classify(windows, assign, hits, second, names, labels, planes, cap=len(wantp) + 9)
    assert (rc, used, text) == (N.KMAN_OK, len(wantp), wantp)
    for keep in ([1, 0, 1, 0, 0, 1], [0] * 6, [1] * 6, [0, 0, 0, 1, 0, 0], [0, 2, 0, 0, 255, 0]):
        for pl in (None, planes):
            w = cc.lines(recs, ltxt, windows, assign, hits, second, pl, keep)
            rc, used, text = _format_classify(windows, assign, hits, second, names, labels, pl, keep, cap=len(w) + 16)
            assert (rc, used, text) == (N.KMAN_OK, len(w), w), keep
    rc, used, text = _format_classify([], [], [], [], [], labels, cap=8)  # zero records
    assert (rc, used, text) == (N.KMAN_OK, 0, b"")
    # an assignment past the labels, and no labels at all
    assert _format_classify(windows, [0, -1, 3, 1, -2, 0], hits, second, names, labels, cap=4096)[0] == N.KMAN_EINVAL
    assert _format_classify(windows, assign, hits, second, names, [], cap=4096)[0] == N.KMAN_EINVAL
    # many records over several host threads, 64 labels
    rng = np.random.default_rng(5)
    n = 20_000
    labels = [b"ref%d" % c for c in range(64)]
    ltxt = [x.decode() for x in labels]
    windows, hits, second = (rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32) for _ in range(3))
    assign = rng.integers(-2, 64, n).astype(np.int32)
    planes = rng.integers(0, 1 << 20, (64, n)).astype(np.uint32)
    names = [b"n%d" % i for i in range(n)]
    recs = [(x.decode(), "") for x in names]
    keep = rng.integers(0, 2, n).astype(np.uint8)
    for pl in (None, planes):
        w = cc.lines(recs, ltxt, windows, assign, hits, second, pl, keep)
        for threads in (1, 4):
            rc, used, text = _format_classify(windows, assign, hits, second, names, labels, pl, keep, cap=len(w),
                                              threads=threads)
            assert (rc, used) == (N.KMAN_OK, len(w)) and text == w


# ------------------------------------------------------------ classify_assign


def test_classify_assign_on_a_grid():
    from kman_amd import engine

    NONE = cc.NONE
    #        windows best hits second
    rows = [(10, 0, 5, 5),       # hits == second: a tie
            (10, 1, 5, 4),       # a margin of 1
            (10, 2, 8, 2),
            (10, 0, 5, 0),       # min_frac 0.5 exactly met
            (10, 1, 4, 0),       # and just missed
            (0, NONE, 0, 0),     # windows == 0, best == NONE
            (7, NONE, 0, 0),     # no hit
            (3, 63, 1, 0),
            (4, 0, 1, 1),
            ((1 << 32) - 1, 5, (1 << 32) - 1, (1 << 32) - 2),
            (100, 3, 50, 49)]
    w, b, h, s = (np.asarray(col, dtype=np.uint32) for col in zip(*rows))
    seen = set()
    for min_hits in (0, 1, 2, 5, 6):
        for min_frac in (0.0, 0.5, 0.8, 1.0):
            for min_margin in (1, 2, 4):
                got = engine.classify_assign(w, b, h, s, min_hits, min_frac, min_margin)
                assert got.dtype == np.int32 and got.shape == (len(rows),)
                want = cc.assign(w, b, h, s, min_hits, min_frac, min_margin)
                assert got.tolist() == want, (min_hits, min_frac, min_margin)
                seen.update(want)
    assert {-1, -2, 0, 1, 2, 5, 63} <= seen
    d = engine.classify_assign(w, b, h, s)  # the defaults: 1 hit, any fraction, a margin of 1
    assert d.tolist() == [-2, 1, 2, 0, 1, -1, -1, 63, -2, 5, 3]
    assert engine.classify_assign(w, b, h, s, 0, 0.0, 1).tolist() == d.tolist()  # (never assigned with 0 hits)
    assert engine.classify_assign(w, b, h, s, 1, 0.5, 1).tolist() == [-2, 1, 2, 0, -1, -1, -1, -1, -1, 5, 3]
    assert engine.classify_assign([], [], [], []).shape == (0,)
    assert (engine.UNASSIGNED, engine.AMBIGUOUS) == (cc.UNASSIGNED, cc.AMBIGUOUS) == (-1, -2)
    for kw in (dict(min_margin=0), dict(min_margin=-1), dict(min_margin=1.5), dict(min_hits=-1), dict(min_hits=True),
               dict(min_frac=1.5), dict(min_frac=-0.1), dict(min_frac=float("nan"))):
        with pytest.raises(AssertionError):
            engine.classify_assign(w, b, h, s, **kw)
    with pytest.raises(AssertionError):
        engine.classify_assign(w, b, h, s[:-1])


# ------------------------------------------------------------- the oracle


HAND_REFS = [[("a", "ACGTA")], [("b", "TTT")], [("c", "CGT"), ("c2", "gggg")]]
HAND_READS = [
    ("flip", "ACGTCGTTTT"),   # ACG(a) CGT(a,c) GTC TCG CGT(a,c) GTT TTT(b) TTT(b)
    ("onlyc", "GGGGG"),       # GGG x3
    ("tie", "CGTN"),          # CGT(a,c)
    ("short", "AC"),
    ("empty", ""),
    ("none", "CCCCC"),
    ("masked", "acgNtttA"),   # ACG(a), TTT(b), TTA
]


def test_helper_on_a_three_reference_example():
    """k = 3, written out by hand: the 3-mer CGT is in references a and c, so
    it votes for both unless --specific, which changes the winner of `flip`."""
    k = 3
    ct = cc.color_table_of(HAND_REFS, k)
    assert ct == {"ACG": 1, "CGT": 1 | 4, "GTA": 1, "TTT": 2, "GGG": 4}
    keys, masks = cc.table_rows(ct)
    assert keys.tolist() == [0b000110, 0b011011, 0b101010, 0b101100, 0b111111] and masks.tolist() == [1, 5, 4, 1, 2]
    pl = cc.planes(HAND_READS, k, ct, 3)
    assert pl.dtype == np.uint32 and pl.tolist() == [[8, 3, 1, 0, 0, 3, 3],   # windows
                                                     [3, 0, 1, 0, 0, 0, 1],   # a
                                                     [2, 0, 0, 0, 0, 0, 1],   # b
                                                     [2, 3, 1, 0, 0, 0, 0]]   # c
    pk = cc.pick(pl[1:])
    N_ = cc.NONE
    assert pk.tolist() == [[0, 2, 0, N_, N_, N_, 0], [3, 3, 1, 0, 0, 0, 1], [2, 0, 1, 0, 0, 0, 1]]
    a = cc.assign(pl[0], pk[0], pk[1], pk[2])
    assert a == [0, 2, -2, -1, -1, -1, -2]
    sp = cc.planes(HAND_READS, k, ct, 3, specific=True)
    assert sp.tolist() == [[8, 3, 1, 0, 0, 3, 3], [1, 0, 0, 0, 0, 0, 1], [2, 0, 0, 0, 0, 0, 1], [0, 3, 0, 0, 0, 0, 0]]
    spk = cc.pick(sp[1:])
    sa = cc.assign(sp[0], spk[0], spk[1], spk[2])
    assert sa == [1, 2, -1, -1, -1, -1, -2]  # `flip` goes from a to b, `tie` from ambiguous to unassigned
    labels = ["a", "b", "c"]
    assert cc.lines(HAND_READS, labels, pl[0], a, pk[1], pk[2]) == (
        b"flip\t8\ta\t3\t2\nonlyc\t3\tc\t3\t0\ntie\t1\t?\t1\t1\nshort\t0\t-\t0\t0\nempty\t0\t-\t0\t0\n"
        b"none\t3\t-\t0\t0\nmasked\t3\t?\t1\t1\n")
    assert cc.lines(HAND_READS[:2], labels, sp[0], sa, spk[1], spk[2], sp[1:]) == (
        b"flip\t8\tb\t2\t1\t1\t2\t0\nonlyc\t3\tc\t3\t0\t0\t0\t3\n")
    assert cc.summary(labels, [3, 1, 2], a) == b"a\t3\t1\nb\t1\t0\nc\t2\t1\n?\t0\t2\n-\t0\t3\n"
    # only two of three colours asked for: bit 2 is ignored, CGT is then specific to a
    two = cc.planes(HAND_READS, k, ct, 2, specific=True)
    assert two.tolist() == [[8, 3, 1, 0, 0, 3, 3], [3, 0, 1, 0, 0, 0, 1], [2, 0, 0, 0, 0, 0, 1]]
    # canonical: ACG/CGT -> ACG, GTA -> GTA (TAC), TTT -> AAA, GGG -> CCC
    cct = cc.color_table_of(HAND_REFS, k, canonical=True)
    assert cct == {"ACG": 1 | 4, "GTA": 1, "AAA": 2, "CCC": 4}
    cpl = cc.planes(HAND_READS, k, cct, 3, canonical=True)
    assert cpl[:, 5].tolist() == [3, 0, 0, 3] and cpl[:, 0].tolist() == [8, 3, 2, 3]
    # -L 2 inside each reference: nothing occurs twice but c2's GGG
    assert cc.color_table_of(HAND_REFS, k, min_count=2) == {"GGG": 4}
    # pick: ties go to the lowest index, one colour has no runner-up
    assert cc.pick([[4, 0], [4, 0], [4, 0]]).tolist() == [[0, cc.NONE], [4, 0], [4, 0]]
    assert cc.pick([[7, 0]]).tolist() == [[0, cc.NONE], [7, 0], [0, 0]]
    text = sc.fasta(HAND_READS)
    import reads_cases as rcs

    files = cc.cut_files(text, rcs.fasta_offsets(text), labels, a, "p", "fa")
    assert sorted(files) == ["p.a.fa", "p.ambiguous.fa", "p.b.fa", "p.c.fa", "p.unassigned.fa"]
    assert files["p.a.fa"] == b">flip\nACGTCGTTTT\n" and files["p.b.fa"] == b""
    assert files["p.ambiguous.fa"] == b">tie\nCGTN\n>masked\nacgNtttA\n"
    assert b"".join(files.values()).count(b">") == len(HAND_READS)
