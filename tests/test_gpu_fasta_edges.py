"""kman_parse_fasta with every event on a chunk, tile or scan-block edge
(tests/fasta_cases.py): engine.parse, kman_parse_fasta_at called directly at
every output alignment, and the chunked loader, each against the numpy oracle
for equality -- counts, codes with their record-start bits, the 64 pad codes,
rec_seq, rec_hdr and the names."""

from __future__ import annotations

import functools
from ctypes import byref, c_void_p

import numpy as np
import pytest

import fasta_cases as fc
import np_oracle

pytestmark = pytest.mark.gpu

from kman_amd import _native as N  # noqa: E402

TILE = fc.TILE
SMALL = fc.small_cases()
PAD = 256   # sentinel bytes after the codes a call may write
RPAD = 16   # sentinel words after a record array
SENT8, SENT64 = 0xA5, 0xA5A5A5A5A5A5A5A5


@pytest.fixture(scope="module")
def dev():
    from kman_amd import engine

    return engine.default_device()


def _expected(text):
    recs = np_oracle.parse_fasta(text)
    codes, rec_seq = np_oracle.codes_of(recs)
    return recs, codes, rec_seq, fc.header_offsets(text), [np_oracle.record_name(t) for t, _ in recs]


@functools.lru_cache(maxsize=None)
def _want(name):
    """The oracle's answer for a small case: computed once, shared, read-only."""
    want = _expected(SMALL[name][0])
    for a in want[1:4]:
        a.setflags(write=False)
    return want


def _check_codes(dev, buf, n_bases, codes_ref):
    got = dev.download(buf, n_bases + 64, np.uint8)
    np.testing.assert_array_equal(got[:n_bases], codes_ref)
    assert np.all(got[n_bases:] == 4)


def _check_parse(dev, text, want):
    from kman_amd import engine

    recs, codes_ref, rec_seq_ref, hdr_ref, names = want
    p = engine.parse(dev, text, "fasta")
    try:
        assert p.n_records == len(recs)
        assert p.n_bases == len(codes_ref)
        _check_codes(dev, p.codes, p.n_bases, codes_ref)
        np.testing.assert_array_equal(p.rec_seq, rec_seq_ref)
        np.testing.assert_array_equal(p.rec_hdr, hdr_ref)
        assert p.names == names
    finally:
        p.free()


# ------------------------------------------------------------- whole parse


@pytest.mark.parametrize("name", list(SMALL))
def test_parse_small_case(dev, name):
    _check_parse(dev, SMALL[name][0], _want(name))


@pytest.mark.parametrize("name", fc.LARGE_NAMES)
def test_parse_large_case(dev, name):
    """More than 1024 tiles: parse_scan_top and bpre[tb / SCAN_T]."""
    text, _ = fc.large_case(name)
    _check_parse(dev, text, _expected(text))


# ------------------------------------------------- kman_parse_fasta_at


def _parse_at(dev, chunk, flags, code_off, rec_cap):
    """kman_parse_fasta_at on buffers pre-filled with 0xA5; -> (rc, n_bases,
    n_records, every byte of the codes buffer, both record arrays whole)."""
    n = len(chunk)
    ncodes = code_off + n + 64 + PAD
    bufs = []
    try:
        for nb in (n + 64, ncodes, 8 * (rec_cap + RPAD), 8 * (rec_cap + RPAD)):
            bufs.append(dev.alloc(nb))
            dev.memset(bufs[-1], SENT8, nb)
        d_text, d_codes, d_hdr, d_seq = bufs
        if n:
            dev.upload(d_text, chunk)
        info = N.ParseInfo()
        rc = N.lib().kman_parse_fasta_at(dev.ctx, c_void_p(d_text.ptr), n, flags, c_void_p(d_codes.ptr), code_off,
                                         c_void_p(d_hdr.ptr), c_void_p(d_seq.ptr), rec_cap, byref(info))
        dev.sync()
        return (rc, int(info.n_bases), int(info.n_records), dev.download(d_codes, ncodes, np.uint8),
                dev.download(d_hdr, rec_cap + RPAD, np.uint64), dev.download(d_seq, rec_cap + RPAD, np.uint64))
    finally:
        for b in bufs:
            b.free()


def _expected_at(chunk, in_record):
    """(codes, rec_seq, rec_hdr) of a chunk; in_record: the chunk continues a
    record, so it is the oracle of ``>x\\n`` + chunk without that record in
    the table and without the mark on its first base."""
    if not in_record:
        _, codes, rec_seq, hdr, _ = _expected(chunk)
        return codes, rec_seq, hdr
    recs = np_oracle.parse_fasta(b">x\n" + chunk)
    codes, rec_seq = np_oracle.codes_of(recs)
    if len(recs[0][1]):
        codes[0] &= 7
    return codes, rec_seq[1:], fc.header_offsets(chunk)


def _check_at(dev, chunk, flags, code_off, want):
    codes_ref, rec_seq_ref, hdr_ref = want
    nb, R = len(codes_ref), len(hdr_ref)
    rc, n_bases, n_records, codes, hdr, seq = _parse_at(dev, chunk, flags, code_off, R + 2)
    assert rc == N.KMAN_OK
    assert (n_bases, n_records) == (nb, R)
    assert np.all(codes[:code_off] == SENT8)
    np.testing.assert_array_equal(codes[code_off:code_off + nb], codes_ref)
    assert np.all(codes[code_off + nb:code_off + nb + 64] == 4)
    assert np.all(codes[code_off + nb + 64:] == SENT8)
    np.testing.assert_array_equal(seq[:R], rec_seq_ref + np.uint64(code_off))
    np.testing.assert_array_equal(hdr[:R], hdr_ref)
    assert np.all(hdr[R:] == SENT64) and np.all(seq[R:] == SENT64)


CODE_OFFS = list(range(16)) + [TILE + 5]
ONE_PER_FAMILY = ["gt_at_16384", "crlf_at_16384", "cr_base_at_16384", "cr_gt_at_16448", "blank4_at_16384",
                  "ws_run_16384_L130_exotic_base", "ws_run_16448_L16394_plain_nl", "long_hdr_letters", "pre_junk_16385",
                  "empty_recs_lf_at_16384", "empty_recs_header_tile", "empty_recs_blank_tile", "gt_inside_16384",
                  "eof_at_16385_base", "eof_lone_gt_last_tile", "loader_blank_chunk"]
AT_CASES = ONE_PER_FAMILY + [n for n in SMALL if n.startswith("hdr_tail_%d_" % TILE)]


def test_at_cases_cover_the_families():
    assert {SMALL[n][1]["family"] for n in AT_CASES} == set(fc.FAMILIES)
    assert sum(n.startswith("hdr_tail") for n in AT_CASES) == 52


@pytest.mark.parametrize("name", AT_CASES)
def test_parse_at_every_alignment(dev, name):
    """code_off at every residue mod 16 (the staging alignment `al`) and past
    one tile; nothing outside [code_off, code_off + n_bases + 64) is written."""
    text = SMALL[name][0]
    _, codes_ref, rec_seq_ref, hdr_ref, _ = _want(name)
    for code_off in CODE_OFFS:
        _check_at(dev, text, 0, code_off, (codes_ref, rec_seq_ref, hdr_ref))


def _continued(text):
    """The text with its first header line turned into bases: a chunk that
    starts inside a record, every later byte at its offset."""
    assert text.startswith(fc.HEAD)
    return b"ACGTACGTNACGTACG\n" + text[len(fc.HEAD):]


@pytest.mark.parametrize("name", [n for n in ONE_PER_FAMILY if SMALL[n][0].startswith(fc.HEAD)]
                         + ["hdr_tail_16384_h1_d7_letters", "hdr_tail_16384_h9_d8_ws", "hdr_tail_16384_h70_d65_letters"])
def test_parse_at_in_record(dev, name):
    chunk = _continued(SMALL[name][0])
    want = _expected_at(chunk, True)
    assert len(want[0]) and not want[0][0] & 8  # the record's bases are counted, its first code is not marked
    for code_off in (0, 5, 16, TILE + 5):
        _check_at(dev, chunk, N.KMAN_PARSE_IN_RECORD, code_off, want)


def test_parse_at_in_record_chunk_starts_with_header(dev):
    text = SMALL["gt_at_16384"][0]
    want = _expected_at(text, True)
    assert int(want[2][0]) == 0 and int(want[1][0]) == 0
    np.testing.assert_array_equal(want[0], _want("gt_at_16384")[1])
    _check_at(dev, text, N.KMAN_PARSE_IN_RECORD, 7, want)


def test_parse_at_without_a_header_and_empty(dev):
    rng = np.random.default_rng(5)
    chunk = fc.seq_text(rng, 3 * TILE + 5, 61, end_nl=False)
    want = _expected_at(chunk, True)
    assert len(want[1]) == 0 and len(want[0]) == len(chunk) - chunk.count(b"\n")
    _check_at(dev, chunk, N.KMAN_PARSE_IN_RECORD, 3, want)
    # empty, in a record: fine, nothing written
    rc, nb, R, codes, hdr, seq = _parse_at(dev, b"", N.KMAN_PARSE_IN_RECORD, 3, 4)
    assert (rc, nb, R) == (N.KMAN_OK, 0, 0)
    assert np.all(codes == SENT8) and np.all(hdr == SENT64) and np.all(seq == SENT64)
    # not in a record: both are a file without a header line
    assert _parse_at(dev, chunk, 0, 3, 4)[0] == N.KMAN_EFORMAT
    assert _parse_at(dev, b"", 0, 3, 4)[0] == N.KMAN_EFORMAT
    _check_at(dev, chunk, N.KMAN_PARSE_IN_RECORD, 0, want)  # the context is still usable


def test_parse_at_record_capacity(dev):
    name = "empty_recs_lf_at_16384"
    text = SMALL[name][0]
    _, codes_ref, rec_seq_ref, hdr_ref, _ = _want(name)
    R = len(hdr_ref)
    assert R > 10
    for cap in (R - 1, 1, 0):
        rc, nb, nr, codes, hdr, seq = _parse_at(dev, text, 0, 9, cap)
        assert rc == N.KMAN_ECAP and nr == R
        assert np.all(codes == SENT8) and np.all(hdr == SENT64) and np.all(seq == SENT64)
    _check_at(dev, text, 0, 9, (codes_ref, rec_seq_ref, hdr_ref))  # the context is still usable


# --------------------------------------------------------- chunked loader


def _check_loaded(dev, text, chunk, want, cut=None):
    from kman_amd import shard

    if cut is not None:
        assert cut in shard.chunk_cuts(shard.BytesReader(text), 0, len(text), chunk)
    recs, codes_ref, rec_seq_ref, _, names = want
    p = shard.load_text(dev, text, chunk)
    try:
        assert p.n_records == len(recs)
        assert p.n_bases == len(codes_ref)
        _check_codes(dev, p.codes, p.n_bases, codes_ref)
        np.testing.assert_array_equal(p.rec_seq, rec_seq_ref)
        assert p.names == names
    finally:
        p.free()


@pytest.mark.parametrize("name", list(SMALL))
def test_loader_tile_chunks(dev, name):
    _check_loaded(dev, SMALL[name][0], TILE, _want(name))


AFTER_HEADER = [n for n in SMALL if n.startswith("gt_at_")] + \
    ["hdr_tail_%d_h%d_d%d_letters" % (TILE, h, d) for h in (1, 2, 9, 70) for d in (0, 1, 8, 9)]


@pytest.mark.parametrize("name", AFTER_HEADER)
def test_loader_cut_after_header(dev, name):
    """The cut falls right after the header line at the edge: the next chunk
    starts with the record's first base, which the loader marks."""
    text, meta = SMALL[name]
    ls = np.nonzero(fc.line_starts(text))[0]
    cut = int(ls[np.searchsorted(ls, meta["at"], side="right")])
    assert text[meta["at"]] == fc.GT and text[cut] in fc.LETTERS
    _check_loaded(dev, text, cut, _want(name), cut=cut)


def test_loader_chunk_of_blank_lines(dev):
    """One chunk ends with the header line, the next holds blank lines only,
    the third starts with the record's first base."""
    text, meta = SMALL["loader_blank_chunk"]
    c = meta["chunk"]
    assert text[c - 1] == 0x0A and not text[c:2 * c].strip(b"\n") and text[c - 2] != 0x0A
    _check_loaded(dev, text, c, _want("loader_blank_chunk"), cut=2 * c)


@pytest.mark.parametrize("X", [x for x in fc.EDGES if x >= TILE - 1])
def test_loader_cut_on_lf_of_crlf(dev, X):
    """The chunk size points at the \\n of a \\r\\n pair: the cut goes after it."""
    name = "crlf_at_%d" % X
    text = SMALL[name][0]
    assert text[X - 1:X + 1] == b"\r\n"
    _check_loaded(dev, text, X, _want(name), cut=X + 1)
