"""`kmer sets` and engine.set_op without a GPU: the command's options, every
refusal raised before any device work or output file, the argument checks of
set_op, the constants of the ABI, and the numpy statement of the set
operations (tests/setop_cases.py) pinned to set arithmetic on the reference's
own `count` lines."""

from __future__ import annotations

import os
import re

import numpy as np
import pytest
from click.testing import CliRunner

import setop_cases as sc
from conftest import GOLDEN


@pytest.fixture()
def inputs(tmp_path):
    fa = tmp_path / "a.fa"
    fa.write_bytes(b">r\nACGTACGTTGCAACGT\n")
    fb = tmp_path / "b.fa"
    fb.write_bytes(b">s\nTTGCAACGTACG\n")
    fq = tmp_path / "c.fq"
    fq.write_bytes(b"@q\nACGTACGTTG\n+\nIIIIIIIIII\n")
    return fa, fb, fq


def test_help_shows_every_option():
    from kman_amd.scripts.kmer import main

    run = CliRunner()
    text = run.invoke(main, ["sets", "--help"]).output
    for opt in ("INPUT_A", "INPUT_B", "OUTPUT", " K", "--op", "intersect", "subtract", "union", "--counts", "left",
                "right", "min", "max", "sum", "-r,", "--reverse", "--canonical", "--format", "-q,", "--min-qual",
                "--phred-offset", "-L,", "--min-count", "-U,", "--max-count"):
        assert opt in text, opt
    assert "sets" in run.invoke(main, ["--help"]).output


REFUSED = {
    "k_1": (["1", "--op", "intersect"], "k must be >= 1"),
    "k_33": (["33", "--op", "intersect"], "K <= 32"),
    "k_40_union": (["40", "--op", "union"], "limit"),
    "canonical_reverse": (["5", "--op", "union", "--canonical", "-r"], "--canonical with -r"),
    "min_qual_without_fastq": (["5", "--op", "subtract", "-q", "20"], "--min-qual"),
    "subtract_counts_right": (["5", "--op", "subtract", "--counts", "right"], "--counts right"),
    "subtract_counts_sum": (["5", "--op", "subtract", "--counts", "sum"], "--counts sum"),
    "union_counts_left": (["5", "--op", "union", "--counts", "left"], "--counts left"),
    "union_counts_min": (["5", "--op", "union", "--counts", "min"], "--counts min"),
    "min_above_max": (["5", "--op", "intersect", "-L", "6", "-U", "5"], "--min-count 6 is greater than --max-count 5"),
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
    out = tmp_path / "out.txt"
    r = CliRunner().invoke(main, ["sets", str(inputs[0]), str(inputs[1]), str(out)] + argv)
    assert isinstance(r.exception, AssertionError), (r.exception, r.output)
    assert msg in str(r.exception)
    assert not out.exists()


def test_min_qual_is_taken_when_one_input_is_fastq(inputs, tmp_path, monkeypatch):
    """-q with one fastq input passes the option checks (it masks that input
    only): the command gets as far as asking for the device."""
    from kman_amd import engine
    from kman_amd.scripts.kmer import main

    class Reached(Exception):
        pass

    def device(*a, **kw):
        raise Reached()

    monkeypatch.setattr(engine, "default_device", device)
    for v in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "KMAN_DIST"):
        monkeypatch.delenv(v, raising=False)
    out = tmp_path / "out.txt"
    for a, b in ((inputs[0], inputs[2]), (inputs[2], inputs[0])):
        r = CliRunner().invoke(main, ["sets", str(a), str(b), str(out), "5", "--op", "intersect", "-q", "20"])
        assert isinstance(r.exception, Reached), (r.exception, r.output)
    r = CliRunner().invoke(main, ["sets", str(inputs[0]), str(inputs[1]), str(out), "5", "--op", "intersect",
                                  "-q", "20", "--format", "fasta"])
    assert isinstance(r.exception, AssertionError) and "--min-qual" in str(r.exception)
    assert not out.exists()


@pytest.mark.parametrize("argv", [["5"], ["5", "--op", "xor"], ["5", "--op", "union", "--counts", "product"],
                                  ["5", "--op", "union", "-L", "0"]])
def test_usage_errors(argv, inputs, tmp_path):
    from kman_amd.scripts.kmer import main

    out = tmp_path / "out.txt"
    r = CliRunner().invoke(main, ["sets", str(inputs[0]), str(inputs[1]), str(out)] + argv)
    assert r.exit_code == 2 and not out.exists()


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
    out = tmp_path / "out.txt"
    r = CliRunner().invoke(main, ["sets", str(inputs[0]), str(inputs[1]), str(out), "5", "--op", "union"])
    assert r.exception is None and r.exit_code == 0 and not out.exists()
    # (a refusal is raised on every rank)
    r = CliRunner().invoke(main, ["sets", str(inputs[0]), str(inputs[1]), str(out), "40", "--op", "union"])
    assert isinstance(r.exception, AssertionError)


class _Stub:
    """A count table that no device call may touch."""

    def __init__(self, k, n=3, count_bytes=4):
        self.k, self.n, self.count_bytes = k, n, count_bytes

    def __getattr__(self, name):
        raise RuntimeError("device buffer %s read before the arguments were checked" % name)


def test_set_op_argument_checks():
    from kman_amd import engine

    a, b = _Stub(21), _Stub(21)
    bad = [
        ("xor", None, 1, None), ("subtract", "right", 1, None), ("subtract", "sum", 1, None),
        ("union", "left", 1, None), ("union", "min", 1, None), ("union", "right", 1, None),
        ("intersect", "any_sum", 1, None), ("intersect", "absent", 1, None), ("intersect", "left", 3, 2),
        ("intersect", "left", 1, 0), ("union", "sum", 1.5, None), ("union", "sum", 1, 2.5),
    ]
    for op, counts, lo, hi in bad:
        with pytest.raises(AssertionError):
            engine.set_op(None, a, b, op, counts, lo, hi)
    for op in ("intersect", "subtract", "union"):
        with pytest.raises(AssertionError, match="different k"):
            engine.set_op(None, a, _Stub(22), op)
    with pytest.raises(AssertionError, match="different k"):
        engine.match_counts(None, a, _Stub(22))
    with pytest.raises(AssertionError, match="match op"):
        engine.match_counts(None, a, b, "xor")
    assert engine.check_set_op("intersect") == "left" and engine.check_set_op("subtract") == "left"
    assert engine.check_set_op("union") == "sum" and engine.check_set_op("union", "max") == "max"
    for op, choices in sc.SET_COUNTS.items():
        assert engine.SET_OPS[op] == choices
        for c in choices:
            assert engine.check_set_op(op, c) == c


def test_constants_match_the_header():
    from kman_amd import _native as N
    from kman_amd import engine

    with open(os.path.join(os.path.dirname(N.HERE), "include", "kman.h")) as fh:
        text = fh.read()
    names = ["KMAN_MATCH_TILE"] + ["KMAN_MATCH_" + op.upper() for op in sc.MATCH_OPS]
    for name in names:
        m = re.search(r"#define\s+%s\s+(\d+)\s" % name, text)
        assert m and int(m.group(1)) == getattr(N, name), name
    assert [getattr(N, n) for n in names[1:]] == list(range(8))  # (setop_cases.MATCH_OPS is in that order)
    assert engine.MATCH_OPS == {op: i for i, op in enumerate(sc.MATCH_OPS)}
    assert "kman_match_counts" in N.SIGNATURES and len(N.SIGNATURES["kman_match_counts"][1]) == 12
    assert "kman_match_counts" in N.header_symbols()
    with open(os.path.join(N.HERE, "csrc", "match.hip")) as fh:
        assert "static_assert(MTILE == KMAN_MATCH_TILE" in fh.read()
    with open(os.path.join(N.HERE, "csrc", "Makefile")) as fh:
        assert "match.hip" in fh.read()


def _ref(name: str) -> bytes:
    with open(os.path.join(GOLDEN, "ref_outputs", name + ".txt"), "rb") as fh:
        return fh.read()


def test_numpy_statement_reproduces_the_reference_lines():
    """A = messy1, B = edge, k = 5: set arithmetic on the reference's own
    lines (dicts) == the numpy statement on their rows, for every op and
    `counts` choice and an abundance range."""
    k = 5
    a_text, b_text = _ref("messy1__count__k5"), _ref("edge__count__k5")
    ak, ac = sc.lines_to_rows(a_text, k)
    bk, bc = sc.lines_to_rows(b_text, k)
    assert (len(ak), len(bk)) == (1018, 24) and np.all(ak[1:] > ak[:-1]) and np.all(bk[1:] > bk[:-1])
    assert sc.rows_to_lines(ak, ac, k) == a_text and sc.rows_to_lines(bk, bc, k) == b_text
    hit, _ = sc.lookup(ak, bk, bc)
    assert int(hit.sum()) == 24  # (mixed: 24 shared rows, 994 of A alone)
    for op, choices in sc.SET_COUNTS.items():
        for counts in choices + (None,):
            for lo, hi in ((1, None), (2, None), (2, 5), (1, 1)):
                want = sc.lines_set_op(a_text, b_text, op, counts, lo, hi)
                gk, gc = sc.set_op(ak, ac, bk, bc, op, counts, lo, hi)
                assert sc.rows_to_lines(gk, gc, k) == want, (op, counts, lo, hi)
                if (lo, hi) == (1, None):
                    assert len(gk) == {"intersect": 24, "subtract": 994, "union": 1018}[op]
    # and with the roles swapped (B's rows all occur in A)
    assert sc.lines_set_op(b_text, a_text, "subtract") == b""
    gk, _ = sc.set_op(bk, bc, ak, ac, "subtract")
    assert len(gk) == 0
    # the eight ops on one shared and one unshared row
    i, j = int(np.nonzero(hit)[0][0]), int(np.nonzero(~hit)[0][0])
    ca_i, ca_j = int(ac[i]), int(ac[j])
    cb_i = int(bc[np.searchsorted(bk, ak[i])])
    want = {"right": (cb_i, 0), "left": (ca_i, 0), "min": (min(ca_i, cb_i), 0), "max": (max(ca_i, cb_i), 0),
            "sum": (ca_i + cb_i, 0), "absent": (0, ca_j), "any_sum": (ca_i + cb_i, ca_j),
            "any_max": (max(ca_i, cb_i), ca_j)}
    for op in sc.MATCH_OPS:
        got = sc.match(ak, ac, bk, bc, op)
        assert (int(got[i]), int(got[j])) == want[op], op
    # saturation of the statement itself
    big = np.asarray([sc.U64_MAX - 1], np.uint64)
    assert int(sc.match([7], big, [7], [5], "sum", 8)[0]) == sc.U64_MAX
    assert int(sc.match([7], big, [7], [5], "sum", 4)[0]) == sc.U32_MAX
    assert int(sc.match([7], [sc.U32_MAX], [7], [5], "any_sum", 4)[0]) == sc.U32_MAX
    assert int(sc.match([7], [sc.U32_MAX], [7], [5], "any_sum", 8)[0]) == sc.U32_MAX + 5
