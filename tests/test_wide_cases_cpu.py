"""The k > 32 reference of the GPU tests (wide_cases.py), pinned with no GPU:
its parse -> windows -> sort -> rle -> text reproduces the reference's own
`kmer count` / `kmer uniq` outputs at k >= 33 (golden sha256), its windows
agree with the numpy oracle where one 64-bit key still holds a k-mer, and
every input builder does what it claims."""

from __future__ import annotations

import json
import os

import numpy as np
import pytest

import wide_cases as wc
from conftest import GOLDEN, sha256_bytes

KS = [33, 34, 48, 63, 64]


def _wide_golden():
    with open(os.path.join(GOLDEN, "manifest.json")) as fh:
        cases = json.load(fh)["cases"]
    return [c for c in cases if c["cmd"] in ("count", "uniq") and c["result"]["ok"] and c["k"] >= 33]


def test_golden_has_wide_cases():
    cases = _wide_golden()
    assert len(cases) >= 12
    assert any("-r" in c["flags"] for c in cases)
    assert {c["cmd"] for c in cases} == {"count", "uniq"}
    assert any(c["k"] > 64 for c in cases) and any(c["k"] <= 64 for c in cases)


@pytest.mark.parametrize("case", _wide_golden(), ids=lambda c: c["name"])
def test_restatement_matches_reference(golden_inputs, case):
    with open(golden_inputs[case["input"]], "rb") as fh:
        text = fh.read()
    got = wc.restate(text, case["k"], case["cmd"], rc="-r" in case["flags"])
    assert sha256_bytes(got) == case["sha256"]


@pytest.mark.parametrize("k", [31, 32])
@pytest.mark.parametrize("flags", [(False, False), (True, False), (False, True), (True, True)],
                         ids=["plain", "rc", "canonical", "rc+canonical"])
def test_windows_match_numpy_oracle(k, flags):
    import inputs
    import np_oracle

    rc, canonical = flags
    text = inputs.messy_records(k, n_records=20, max_len=3000)
    keys, pos = np_oracle.stream_kmers(np_oracle.parse_fasta(text), k, rc=rc, canonical=canonical)
    ws = wc.windows(wc.parse(text), k, rc, canonical)
    assert len(ws) == len(keys) > 1000
    assert [wc.to_words(w)[0] for w, _ in ws] == [int(x) for x in keys]
    assert [p for _, p in ws] == [int(x) for x in pos]
    # the record table of the parse
    recs = wc.parse(text)
    assert [n for n, _ in recs] == [np_oracle.record_name(t) for t, _ in np_oracle.parse_fasta(text)]
    assert wc.rec_starts(recs) == [int(x) for x in np_oracle.codes_of(np_oracle.parse_fasta(text))[1]]


@pytest.mark.parametrize("k", [2, 31, 32, 33, 64, 65, 96, 97, 129])
def test_words_round_trip(k):
    W = wc.nwords(k)
    for kmer in (b"A" * k, b"T" * k, wc.clean(k, k), b"C" + b"A" * (k - 1), b"A" * (k - 1) + b"G"):
        w = wc.to_words(kmer)
        assert len(w) == W == (k + 31) // 32
        assert wc.from_words(w, k) == kmer
        # MSB-first: the k-mer read as one base-4 number, cut into a head word and 32-base words
        whole = 0
        for c in kmer:
            whole = whole * 4 + b"ACGT".index(c)
        again = 0
        for j, x in enumerate(w):
            again = (again << 64) | x if j else x
        assert again == whole
    assert wc.to_words(b"A" * k) == (0,) * W
    h = k - 32 * (W - 1)
    assert wc.to_words(b"T" * k) == ((1 << (2 * h)) - 1,) + (wc.ONES,) * (W - 1)
    # word order == str order
    a, b = wc.clean(k, "a"), wc.clean(k, "b")
    assert (a < b) == (wc.to_words(a) < wc.to_words(b))


def test_rle_and_writers_by_hand():
    rows = [b"AA", b"AA", b"AC", b"GT", b"GT", b"GT", b"TT"]
    vals = [10, 11, 12, 13, 14, 15, 16]
    assert wc.rle(rows, vals, "count") == ([b"AA", b"AC", b"GT", b"TT"], [2, 1, 3, 1])
    assert wc.rle(rows, vals, "uniq") == ([b"AC", b"TT"], [12, 16])
    assert wc.rle([], [], "count") == ([], [])
    assert wc.count_text([b"AC", b"TT"], [1, 10], 2) == b"AC\t1\nTT\t10\n"
    # records of 5, 0 and 7 bases: an empty record owns nothing
    assert wc.uniq_text([b"AC", b"TT"], [(3 << 1) | 1, 6 << 1], 2, [b"x", b"", b"z"], [0, 5, 5]) == \
        b">x:3-5:-\nAC\n>z:1-3:+\nTT\n"
    assert wc.revcomp(b"AACG") == b"CGTT"
    recs = wc.parse(b"skip\n>r1 d\nACgt\r\nNN A\n\n>r2\tx\n>r3\rTT\n")
    assert recs == [(b"r1", b"ACgtNNA"), (b"r2\tx", b""), (b"r3", b"TT")]
    assert wc.rec_starts(recs) == [0, 7, 7]
    assert wc.parse(wc.fasta(recs)) == recs
    assert wc.windows(recs, 2, rc=True) == [(b"AC", 0), (b"GT", 1), (b"CG", 2), (b"CG", 3), (b"GT", 4), (b"AC", 5),
                                           (b"TT", 14), (b"AA", 15)]
    assert wc.windows(recs, 2, canonical=True) == wc.windows(recs, 2, rc=True, canonical=True) == \
        [(b"AC", 0), (b"CG", 2), (b"AC", 4), (b"AA", 14)]


@pytest.mark.parametrize("k", KS)
def test_event_builders(k):
    full = wc.SEQ_LEN3 - k + 1
    assert wc.lengths(k)[0] == k - 1 and not wc.valid_starts([(b"s", wc.clean(k - 1, 0))], k)
    assert len(wc.valid_starts([(b"s", wc.clean(k, 0))], k)) == 1
    offs = wc.event_offsets(k)
    assert len(offs) == 18 and wc.TILE in offs and 2 * wc.TILE - k in offs and 2 * wc.TILE + k - 1 in offs
    for at in offs:
        recs = wc.with_n(at)
        assert recs[0][1][at:at + 1] == b"N" and recs[0][1].count(b"N") == 1 and len(recs[0][1]) == wc.SEQ_LEN3
        starts = {g for g, _ in wc.valid_starts(recs, k)}
        assert starts == set(range(full)) - set(range(at - k + 1, at + 1))
        recs = wc.with_start(at)
        assert wc.rec_starts(recs) == [0, at] and sum(len(s) for _, s in recs) == wc.SEQ_LEN3
        starts = {g for g, _ in wc.valid_starts(recs, k)}
        assert starts == set(range(full)) - set(range(at - k + 1, at))
        assert wc.parse(wc.fasta(recs)) == recs
    for second in (False, True):
        at = wc.TILE - 40
        none = {g for g, _ in wc.valid_starts(wc.two_events(k, k - 1, at, second), k)}
        one = {g for g, _ in wc.valid_starts(wc.two_events(k, k, at, second), k)}
        # windows that start after the first event and end before the second (at at + 1 + between)
        assert not [g for g in none if at < g < at + k]
        assert [g for g in one if at < g < at + k + 1] == [at + 1]
        assert (at + k in none) == second and (at + k + 1 in one) == second  # a record start opens a window


@pytest.mark.parametrize("k", KS)
def test_key_builders(k):
    at = wc.TILE - 3
    if k % 2 == 0:
        p = wc.palindrome(k)
        assert len(p) == k and wc.revcomp(p) == p
        recs = wc.embed(p, at)
        assert recs[0][1][at:at + k] == p
        assert (p, at << 1) in wc.windows(recs, k, canonical=True)
    if k < 64:
        m = k - 32
        f, r = wc.hi_tie(k, True), wc.hi_tie(k, False)
        for w in (f, r):
            assert len(w) == k and w[:m] == wc.revcomp(w[-m:])
            assert wc.to_words(w)[0] == wc.to_words(wc.revcomp(w))[0]
            assert wc.to_words(w)[1] != wc.to_words(wc.revcomp(w))[1]
        assert f < wc.revcomp(f) and wc.revcomp(r) < r
        assert (f, at << 1) in wc.windows(wc.embed(f, at), k, canonical=True)
        assert (wc.revcomp(r), at << 1) in wc.windows(wc.embed(r, at), k, canonical=True)
    for c in (b"A", b"T"):
        recs = wc.embed(c * k, at)
        assert (c * k, at << 1) in wc.windows(recs, k)
    assert wc.to_words(b"T" * 64) == (wc.ONES, wc.ONES)


@pytest.mark.parametrize("tile,per", [(wc.RLE_WIDE_TILE, wc.RLE_WIDE_PER), (wc.RLE_WORDS_TILE, wc.RLE_WORDS_PER)])
@pytest.mark.parametrize("n", [0, 1, 2, 17, 2049, 4097, 3 * 4096 + 1])
def test_rle_layouts(n, tile, per):
    lay = wc.rle_layouts(n, tile, per)
    if n == 0:
        assert lay == {"empty": []}
        return

    def bounds(sizes):  # [(first row, last row)]
        out, at = [], 0
        for m in sizes:
            out.append((at, at + m - 1))
            at += m
        return out

    assert lay["distinct"] == [1] * n and lay["equal"] == [n]
    b = bounds(lay["straddle2"])
    for t in range(tile, n, tile):
        assert (t - 1, t) in b
    if n > tile:
        a, e = max(bounds(lay["long"]), key=lambda x: x[1] - x[0])
        assert a == tile - 1 and e == min(n - 1, 3 * tile)
    b = bounds(lay["singles"])
    for t in range(0, n, tile):
        for i in (t, t + tile - 1, t + 5 * per, t + 6 * per - 1):
            if i < n:
                assert (i, i) in b
    if n >= 3:
        assert bounds(lay["tail"])[-1] == (n - 3, n - 1)
    for W in (1, 2, 5):
        for vary in ["all"] + list(range(W)):
            sizes = lay["singles"]
            rows = wc.rle_rows(sizes, W, vary)
            assert len(rows) == n and all(len(r) == W for r in rows)
            assert wc.rle(rows, None, "count")[1] == sizes
            if vary != "all":
                assert rows == sorted(rows)
                for x, y in zip(rows, rows[1:]):
                    assert all(x[q] == y[q] for q in range(W) if q != vary)
    rows = wc.rle_rows(lay["distinct"], 2, "all", ones="both")
    assert rows[0] == (wc.ONES, wc.ONES) == rows[-1]
    assert n < 3 or all(r != (wc.ONES, wc.ONES) for r in rows[1:-1])


def test_row_arrays_are_uint64():
    rows = wc.rle_rows([1, 2, 1], 3, "all", ones="last")
    a = np.array(rows, dtype=np.uint64)
    assert a.shape == (4, 3) and [tuple(int(x) for x in r) for r in a] == rows
