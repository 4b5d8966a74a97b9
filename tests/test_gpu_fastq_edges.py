"""kman_parse_fastq / kman_parse_fastq_q with every event of the parse and of
the quality mask on a chunk, tile or scan-block edge (tests/fastq_edge_cases.py;
its coverage conditions are asserted in test_fastq_edge_cases_cpu.py).  The
entry points are called through ctypes on buffers filled with a sentinel and
compared for equality with the statement: counts, codes with their record-start
bits, the 64 pad codes, rec_seq, rec_hdr (every header's offset, not only that
it holds an ``@``), n_masked, and nothing written past any of them.  Every
text also runs once under a threshold byte, its quality lines regenerated."""

from __future__ import annotations

import functools
from ctypes import byref, c_uint64, c_void_p

import numpy as np
import pytest

import fastq_edge_cases as fe
import np_oracle

pytestmark = pytest.mark.gpu

from kman_amd import _native as N  # noqa: E402

TILE = fe.TILE
SMALL = fe.small_cases()
VALID = [n for n, (_, m) in SMALL.items() if m.get("message") is None]
ERRORS = [n for n, (_, m) in SMALL.items() if m.get("message") is not None]
PAD = 256   # sentinel bytes after the codes a call may write
RPAD = 16   # sentinel words after a record array
SENT8, SENT64 = 0xA5, 0xA5A5A5A5A5A5A5A5


@pytest.fixture(scope="module")
def dev():
    from kman_amd import engine

    return engine.default_device()


def _text(name: str, masked: bool):
    """(text, threshold byte): a qmask case carries its own quality bytes and
    threshold; any other case, run masked, gets its quality lines regenerated
    from {T - 1, T}."""
    text, meta = SMALL[name] if name in SMALL else fe.large_case(name)
    if not masked:
        return text, 0
    if "T" in meta:
        return text, meta["T"]
    return fe.requal(text), fe.T_PLAIN


def _expected(text, qbyte):
    R, codes, rec_seq, n_masked = fe.expected(text, qbyte)
    hdr = fe.header_offsets(text)
    for a in (codes, rec_seq, hdr):
        a.setflags(write=False)
    return R, codes, rec_seq, hdr, n_masked


@functools.lru_cache(maxsize=None)
def _want(name: str, masked: bool):
    """The statement's answer for a small case: computed once, shared, read-only."""
    return _expected(*_text(name, masked))


def _parse(dev, text: bytes, qbyte: int, rec_cap: int):
    """One call on buffers pre-filled with 0xA5 -> (rc, message, n_bases,
    n_records, n_masked, every byte of the codes buffer, both record arrays
    whole).  qbyte 0 goes to kman_parse_fastq, any other to kman_parse_fastq_q."""
    n = len(text)
    bufs = []
    try:
        for nb in (n + 64, n + 64 + PAD, 8 * (rec_cap + RPAD), 8 * (rec_cap + RPAD)):
            bufs.append(dev.alloc(nb))
            dev.memset(bufs[-1], SENT8, nb)
        d_text, d_codes, d_hdr, d_seq = bufs
        dev.upload(d_text, text)
        info, masked = N.ParseInfo(), c_uint64(0)
        args = (dev.ctx, c_void_p(d_text.ptr), n, c_void_p(d_codes.ptr), c_void_p(d_hdr.ptr), c_void_p(d_seq.ptr),
                rec_cap, byref(info))
        if qbyte:
            rc = N.lib().kman_parse_fastq_q(*args, qbyte, byref(masked))
        else:
            rc = N.lib().kman_parse_fastq(*args)
        msg = N.lib().kman_last_error(dev.ctx).decode(errors="replace") if rc != N.KMAN_OK else ""
        dev.sync()
        return (rc, msg, int(info.n_bases), int(info.n_records), int(masked.value),
                dev.download(d_codes, n + 64 + PAD, np.uint8), dev.download(d_hdr, rec_cap + RPAD, np.uint64),
                dev.download(d_seq, rec_cap + RPAD, np.uint64))
    finally:
        for b in bufs:
            b.free()


def _check(dev, text, qbyte, want):
    R, codes_ref, rec_seq_ref, hdr_ref, n_masked = want
    nb = len(codes_ref)
    # (rec_cap == R: just enough)
    rc, msg, n_bases, n_records, got_masked, codes, hdr, seq = _parse(dev, text, qbyte, R)
    assert (rc, msg) == (N.KMAN_OK, "")
    assert (n_records, n_bases) == (R, nb)
    np.testing.assert_array_equal(codes[:nb], codes_ref)
    assert np.all(codes[nb:nb + 64] == 4)
    assert np.all(codes[nb + 64:] == SENT8)
    np.testing.assert_array_equal(seq[:R], rec_seq_ref)
    np.testing.assert_array_equal(hdr[:R], hdr_ref)
    assert np.all(hdr[R:] == SENT64) and np.all(seq[R:] == SENT64)
    assert got_masked == n_masked


# ------------------------------------------------------------- small cases


@pytest.mark.parametrize("name", VALID)
def test_parse_case(dev, name):
    text, _ = _text(name, False)
    _check(dev, text, 0, _want(name, False))


@pytest.mark.parametrize("name", VALID)
def test_parse_case_under_a_threshold(dev, name):
    text, qbyte = _text(name, True)
    want = _want(name, True)
    if SMALL[name][1]["family"] != "qmask":
        assert len(want[1]) < 8 or 0 < want[4] < len(want[1])  # (some codes masked, some not)
    _check(dev, text, qbyte, want)


def test_masked_record_start_reads_12(dev):
    name = "qmask_g7_record_start"
    text, qbyte = _text(name, True)
    i = SMALL[name][1]["code12"]
    assert _want(name, True)[1][i] == 12 and _want(name, False)[1][i] & 8
    rc, _, _, _, _, codes, _, _ = _parse(dev, text, qbyte, _want(name, True)[0])
    assert rc == N.KMAN_OK and codes[i] == 12 and np.all(codes[i - 16:i] < 12)


# ------------------------------------------------------------ large cases


@pytest.mark.parametrize("name", fe.LARGE_NAMES)
def test_parse_large_case(dev, name):
    """More than 1024 tiles: fq_scan_top and bpre[tb / SCAN_T], a line start
    within a byte of the block edge, lines before it not a multiple of four."""
    masked = "T" in fe.large_case(name)[1]
    text, qbyte = _text(name, masked)
    _check(dev, text, qbyte, _expected(text, qbyte))


# ------------------------------------------------------------------ errors


@pytest.mark.parametrize("name", ERRORS)
@pytest.mark.parametrize("qbyte", [0, fe.T_PLAIN], ids=["plain", "threshold"])
def test_error_case(dev, name, qbyte):
    text, meta = SMALL[name]
    R = len(fe.header_offsets(text))
    rc, msg, n_bases, n_records, n_masked, _, hdr, seq = _parse(dev, text, qbyte, R)
    assert (rc, msg) == (N.KMAN_EFORMAT, meta["message"])
    assert (n_bases, n_records, n_masked) == (0, 0, 0)
    assert np.all(hdr[R:] == SENT64) and np.all(seq[R:] == SENT64)
    # the next parse on the same context is correct
    ok = "ls_sequence_crlf_at_64"
    good, q = _text(ok, bool(qbyte))
    _check(dev, good, q, _want(ok, bool(qbyte)))


# ---------------------------------------------------------- record capacity


@pytest.mark.parametrize("name", ["multi_run_tiny_at_16384_p0", "eof_cut_record", "eof_blank_tiles"])
def test_record_capacity(dev, name):
    text, _ = _text(name, False)
    want = _want(name, False)
    R = want[0]
    assert R > 10
    for qbyte in (0, fe.T_PLAIN):
        rc, msg, n_bases, n_records, _, codes, hdr, seq = _parse(dev, text, qbyte, R - 1)
        assert rc == N.KMAN_ECAP and msg == "record capacity %d < %d" % (R - 1, R)
        assert (n_bases, n_records) == (0, 0)
        assert np.all(codes == SENT8) and np.all(hdr == SENT64) and np.all(seq == SENT64)
    _check(dev, text, 0, want)  # rec_cap == R passes, on the same context


# ------------------------------------------------------------ engine level

ONE_PER_FAMILY = ["ls_quality_crlf_at_16384", "split_crlf_sequence_at_16384", "lone_cr_plus_at_16448", "emit_c1_hi",
                  "multi_run_tiny_at_16384_p2", "multi_run_spaces_at_16384_p1", "trailing_ws_16384_x1c_iii",
                  "eof_at_16385_crlf", "eof_blank_tiles", "eof_cut_record", "qmask_g2_tile1", "qmask_g6_full_tile",
                  "err_valid_seq_crlf_qual_lf"]


def test_engine_cases_cover_the_families():
    assert {SMALL[n][1]["family"] for n in ONE_PER_FAMILY} | {"scan_block"} == set(fe.FAMILIES)


@pytest.mark.parametrize("masked", [False, True], ids=["plain", "threshold"])
@pytest.mark.parametrize("name", ONE_PER_FAMILY)
def test_engine_parse_fastq(dev, name, masked):
    """The host side sees the same offsets: names and names_blob come from rec_hdr."""
    from kman_amd import engine

    text, qbyte = _text(name, masked)
    assert qbyte in (0, fe.T_PLAIN)
    R, codes_ref, rec_seq_ref, hdr_ref, n_masked = _want(name, masked)
    names = [np_oracle.record_name(t) for t, _ in np_oracle.parse_fasta(fe.fq.fastq_to_fasta(text))]
    p = engine.parse_fastq(dev, text, qbyte - 33 if qbyte else 0, 33)
    try:
        assert (p.n_records, p.n_bases, p.n_masked) == (R, len(codes_ref), n_masked)
        got = dev.download(p.codes, p.n_bases + 64, np.uint8)
        np.testing.assert_array_equal(got[:p.n_bases], codes_ref)
        assert np.all(got[p.n_bases:] == 4)
        np.testing.assert_array_equal(p.rec_seq, rec_seq_ref)
        np.testing.assert_array_equal(p.rec_hdr, hdr_ref)
        assert p.names == names
        assert len(p.name_off) == R + 1 and p.names_blob == b"".join(names)
    finally:
        p.free()


def test_engine_errors(dev):
    from kman_amd import engine

    for name in ("err_rule3_straddles_tile", "err_two_offenders_lower_record", "err_trailing_ws_16384_x09_iv"):
        text, meta = SMALL[name]
        for min_qual in (0, 20):
            with pytest.raises(AssertionError) as e:
                engine.parse_fastq(dev, text, min_qual)
            assert str(e.value) == meta["message"]
