"""The FASTA edge cases (tests/fasta_cases.py) without a GPU: every case's
premise holds of its text, the second statement of the parse equals the numpy
oracle on all of them and reproduces the reference's own digests
(tests/golden/fasta_edges.json), and the case set tells a handful of naive
parsers from the right one -- the kernel is never made wrong on purpose, so
the discriminating power of the cases is measured here."""

from __future__ import annotations

import json
import os
import re

import numpy as np
import pytest

import fasta_cases as fc
import np_oracle
from conftest import GOLDEN

TILE, BLOCK = fc.TILE, fc.BLOCK
WS = b" \t\n\x0b\x0c\r\x1c\x1d\x1e\x1f"
EXOTIC = b"\t\x0b\x0c\x1c\x1d\x1e\x1f"


@pytest.fixture(scope="module")
def small():
    return fc.small_cases()


@pytest.fixture(scope="module")
def truth(small):
    """name -> statement(text), computed once and left unchanged."""
    return {name: fc.statement(text) for name, (text, _) in small.items()}


# ---------------------------------------------------------------- premises


def _is(text, at, what):
    if what is None:
        return True
    if what == "base":
        return text[at] in fc.LETTERS
    return text[at:at + 1] == what.encode()


def _check_meta(name, text, meta):
    at = meta["at"]
    assert max(text) < 0x80, name
    assert _is(text, at, meta["byte"]), name
    assert at == 0 or _is(text, at - 1, meta["before"]), name
    for t in meta.get("fast_tiles") or []:
        assert fc.plain_tile(text, t), (name, t)
    if "length" in meta:
        assert len(text) == meta["length"], name


def test_premises_small(small):
    assert len(small) == len(set(small))
    fams = {}
    for name, (text, meta) in small.items():
        _check_meta(name, text, meta)
        assert len(text) <= 4 * TILE + 1024, name  # (four tiles; the header that ends a tile needs a line after it)
        fams.setdefault(meta["family"], []).append(name)
        fam, at = meta["family"], meta["at"]
        if fam == "hdr_tail":
            line = text[at:meta["last"] + 1]
            assert b"\n" not in line and b"\r" not in line and text[meta["last"] + 1] == 0x0A, name
            # the tile after the edge stays on the fast path whenever the header's tail holds letters only
            if name.endswith("letters") or "_h9_" in name or "_h70_" in name:
                assert meta["fast_tiles"] == [(at + TILE - 1) // TILE], name
        elif fam == "crlf_at" and name.startswith(("crlf_at", "cr_base")) and at % TILE == 0:
            assert meta["fast_tiles"] == [at // TILE], name
        elif fam == "ws_run":
            run = text[at:at + meta["run"]]
            assert not run.strip(b" " + EXOTIC) and run[:1] == b"\t", name
            after = text[at + meta["run"]:at + meta["run"] + 1]
            assert {"nl": after == b"\n", "base": after != b"" and after in fc.LETTERS, "eof": after == b""}[meta["end"]]
        elif fam == "long_hdr" and "last" in meta:
            assert text[meta["last"] + 1] == 0x0A and not text[at + 1:meta["last"] + 1].strip(b"ACGTNacgtnXYZ "), name
        elif fam == "pre_junk":
            assert int(fc.header_offsets(text)[0]) == at, name
            if at > 200:
                assert b"xx>yy\n" in text[:at] and b"\n\n" in text[:at], name
        elif fam == "empty_recs" and "only_tile" in meta:
            t = meta["only_tile"]
            tile = text[t * TILE:(t + 1) * TILE]
            if name == "empty_recs_header_tile":
                assert len(tile.split(b"\n")) == TILE // 8 + 1 and all(ln[:1] == b">" for ln in tile.split(b"\n")[:-1])
            else:
                assert not tile.strip(b" \r\n"), name
        elif fam == "gt_inside":
            assert at not in fc.header_offsets(text).tolist(), name
        elif fam == "loader":
            c = meta["chunk"]
            assert text[c - 1] == 0x0A and not text[c:2 * c + 1].strip(b"\n"), name
    assert set(fams) == set(fc.FAMILIES)
    for x in fc.EDGES:
        for fam in ("gt_at", "crlf_at", "blank_at", "pre_junk", "empty_recs", "gt_inside"):
            assert any(small[n][1]["at"] == x for n in fams[fam]), (fam, x)


@pytest.mark.parametrize("name", fc.LARGE_NAMES)
def test_large_case_premises_and_oracle(name):
    text, meta = fc.large_case(name)
    _check_meta(name, text, meta)
    assert 17 << 20 <= len(text) <= 18 << 20 and len(text) > BLOCK + TILE
    recs, hdr = fc.statement(text)
    assert np_oracle.parse_fasta(text) == recs
    b = np.frombuffer(text, np.uint8)
    assert len(hdr) == len(recs) and np.all(b[hdr.astype(np.int64)] == fc.GT)
    if name != "big_crlf_block_no_hdr_after":
        assert meta["at"] in hdr.tolist()
    if "last" in meta:
        assert meta["at"] < BLOCK <= meta["last"] and b"\n" not in text[meta["at"]:meta["last"] + 1]
    if "first_header" in meta:
        assert int(hdr[0]) == meta["first_header"] > BLOCK
        assert text.count(b">", 0, BLOCK) > 100 and text[:BLOCK].count(b"\n") > 200_000
    if "no_header_from" in meta:
        assert hdr.tolist() == [0] and text.find(b">", 1) == -1


# ------------------------------------------------------- oracle agreement


def test_statement_equals_oracle_small(small, truth):
    for name, (text, _) in small.items():
        recs, hdr = truth[name]
        assert np_oracle.parse_fasta(text) == recs, name
        # a `>` starts a line after \n, after \r (whether or not a \n follows the \r, none does here) and at byte 0
        assert hdr.tolist() == [m.end() - 1 for m in re.finditer(rb"(?:\A|[\r\n])>", text)], name
        assert len(hdr) == len(recs), name


def test_statement_reproduces_the_reference(small, truth):
    """The digests the reference's own parser gave (gen_fasta_edges.py)."""
    with open(os.path.join(GOLDEN, "fasta_edges.json")) as fh:
        fx = json.load(fh)
    assert set(fx["digests"]) | set(fx["left_out"]) == set(small)
    assert not set(fx["digests"]) & set(fx["left_out"])
    assert set(fx["left_out"]) == {n for n, (text, _) in small.items() if fc.reference_loops(text)}
    assert len(fx["digests"]) > 300
    for name, want in fx["digests"].items():
        assert fc.digest(truth[name][0]) == want, name


def test_statement_without_a_header():
    for text in (b"", b"ACGT\n", b"x>y\n"):
        with pytest.raises(AssertionError):
            fc.statement(text)


# ------------------------------------------------- discriminating power
#
# Naive parsers, none of them project code.  Each is the statement with one
# mistake a byte-parallel parser can make at a chunk, tile or block edge.
# (One more was considered: "\r at X - 1 and \n at X taken as two line ends
# when X is a multiple of 64".  It only adds an empty line, which changes no
# record, no base and no header offset, so no input can tell it apart.)


def _ulines(text):
    """(offset, content) of every universal-newline line."""
    st = np.nonzero(fc.line_starts(text))[0].tolist() + [len(text)]
    return [(a, text[a:b].rstrip(b"\r\n")) for a, b in zip(st, st[1:])]


def _assemble(events, keep_pre=False):
    recs = []
    for kind, val in events:
        if kind == "h":
            recs.append([val.rstrip(WS), []])
        elif recs or keep_pre:
            if not recs:
                recs.append([b"", []])
            recs[-1][1].append(val)
    return [(t, b"".join(s).replace(b" ", b"").replace(b"\r", b"")) for t, s in recs]


def _right(text):
    return _assemble(("h", ln[1:]) if ln[:1] == b">" else ("s", ln.rstrip(WS)) for _, ln in _ulines(text))


def naive_lf_only(text):
    """Line ends on \\n only."""
    lines = text.split(b"\n")
    return _assemble(("h", ln[1:]) if ln[:1] == b">" else ("s", ln.rstrip(WS)) for ln in lines)


def naive_any_gt(text):
    """Any `>` opens a header."""
    ev = []
    for _, ln in _ulines(text):
        i = ln.find(b">")
        if i < 0:
            ev.append(("s", ln.rstrip(WS)))
        else:
            ev += [("s", ln[:i].rstrip(WS)), ("h", ln[i + 1:])]
    return _assemble(ev)


def _naive_reset(text, period):
    """The state forgotten (back to "sequence line") at every multiple of
    `period`: the rest of a header line is read as bases, and so is whatever
    precedes the first header from there on."""
    ev, seen = [], False
    for a, ln in _ulines(text):
        m = -(-(a + 1) // period) * period  # the first multiple above a
        if ln[:1] == b">":
            seen = True
            if m < a + len(ln):
                ev += [("h", ln[1:m - a]), ("s", ln[m - a:].rstrip(WS))]
            else:
                ev.append(("h", ln[1:]))
        elif seen:
            ev.append(("s", ln.rstrip(WS)))
        elif a + len(ln) > period:
            ev.append(("s", ln[max(0, period - a):].rstrip(WS)))
    return _assemble(ev, keep_pre=True)


def naive_tile_reset(text):
    return _naive_reset(text, TILE)


def naive_block_reset(text):
    return _naive_reset(text, BLOCK)


def naive_chunk_rstrip(text):
    """rstrip looks no further than the 64-byte chunk that holds the
    whitespace: a tab is kept only if a non-blank follows in its own chunk."""
    ev = []
    for a, ln in _ulines(text):
        if ln[:1] == b">":
            ev.append(("h", ln[1:]))
            continue
        if any(c in ln for c in EXOTIC):
            out = bytearray()
            for c0 in range(a - a % fc.CHUNK, a + len(ln), fc.CHUNK):
                seg = ln[max(c0, a) - a:c0 + fc.CHUNK - a]
                body = seg.rstrip(WS)
                out += body + seg[len(body):].translate(None, EXOTIC)
            ln = bytes(out)
        ev.append(("s", ln.rstrip(b" \r\n")))
    return _assemble(ev)


def naive_tabs_dropped(text):
    """Every whitespace byte dropped, trailing or not."""
    return _assemble(("h", ln[1:]) if ln[:1] == b">" else ("s", ln.translate(None, WS)) for _, ln in _ulines(text))


def naive_pre_kept(text):
    """Lines before the first header kept as bases."""
    return _assemble((("h", ln[1:]) if ln[:1] == b">" else ("s", ln.rstrip(WS)) for _, ln in _ulines(text)),
                     keep_pre=True)


# parser -> the families it concerns, and the cases that must all expose it
NAIVE = {
    naive_lf_only: (["crlf_at", "empty_recs"], lambda n, m: n.startswith(("cr_gt_at", "empty_recs_cr"))),
    naive_any_gt: (["gt_inside", "pre_junk"], lambda n, m: m["family"] == "gt_inside" or
                   (m["family"] == "pre_junk" and m["at"] > 200)),
    naive_tile_reset: (["hdr_tail", "long_hdr", "pre_junk"], lambda n, m: (m["family"] == "hdr_tail" and "_d0_" not in n)
                       or n.startswith("long_hdr_") or (m["family"] == "pre_junk" and m["at"] > TILE + 200)),
    naive_chunk_rstrip: (["ws_run"], lambda n, m: m["family"] == "ws_run" and m["end"] == "base" and m["run"] >= 65),
    naive_tabs_dropped: (["ws_run"], lambda n, m: m["family"] == "ws_run" and m["end"] == "base"),
    naive_pre_kept: (["pre_junk"], lambda n, m: m["family"] == "pre_junk"),
}


def test_naive_helpers_are_right_when_not_naive(small, truth):
    """The line walker under the naive parsers is itself the statement."""
    for name, (text, _) in small.items():
        assert _right(text) == truth[name][0], name


@pytest.mark.parametrize("parser", list(NAIVE), ids=lambda f: f.__name__)
def test_cases_expose_naive_parser(small, truth, parser):
    families, must = NAIVE[parser]
    exposed = {}
    for name, (text, meta) in small.items():
        differs = parser(text) != truth[name][0]
        if differs:
            exposed.setdefault(meta["family"], []).append(name)
        if must(name, meta):
            assert differs, name
    for fam in families:
        assert exposed.get(fam), fam


def test_large_cases_expose_block_reset_and_lost_pre():
    """The same mistakes at the 16 MiB scan-block edge: only a large case shows them."""
    for name, parsers in (("big_hdr_spans_block", [naive_block_reset]),
                          ("big_pre_block", [naive_block_reset, naive_pre_kept])):
        text, _ = fc.large_case(name)
        want = fc.statement(text)[0]
        for p in parsers:
            assert p(text) != want, (name, p.__name__)
