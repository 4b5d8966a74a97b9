"""FASTQ quality threshold on the GPU: kman_parse_fastq_q (fq_qmask) against
the FASTA oracles run on the masked records (fastq_qual_cases.mask_fastq), the
extract kernels after masking, the commands, the errors and the API."""

from __future__ import annotations

import functools
import gzip
import os
import subprocess
import sys

import numpy as np
import pytest

import fastq_cases as fq
from conftest import ROOT
from fastq_qual_cases import mask_fastq

pytestmark = pytest.mark.gpu

TILE = 16384

# (min_qual, phred_offset): thresholds '"', '5', 'J', '~' and, at offset 64, 'J'
THRESHOLDS = [(1, 33), (20, 33), (41, 33), (93, 33), (10, 64)]


@pytest.fixture(scope="module")
def dev():
    from kman_amd import engine

    return engine.default_device()


def _one_read(n: int, seed: int = 9) -> bytes:
    rng = np.random.default_rng(seed)
    return fq.record(b"big one", fq.seq_of(rng, n), fq.qual_of(rng, n))


def _first_base_masked() -> bytes:
    """Reads whose first quality byte is '!' (and some whose only one is)."""
    rng = np.random.default_rng(21)
    out = []
    for i, n in enumerate([1, 5, 64, 1, 150, 63, 2, 65, 1]):
        out.append(fq.record(b"m%d" % i, fq.seq_of(rng, n), fq.qual_of(rng, n, b"!")))
    return b"".join(out)


def _wide_quality_bytes() -> bytes:
    """Quality bytes from all of 0x21..0xff: thresholds above 0x80 split them."""
    rng = np.random.default_rng(22)
    alphabet = np.arange(0x21, 0x100, dtype=np.uint8)
    out = []
    for i, n in enumerate([150, 1, 64, 65, 300, 20, 63, 151]):
        out.append(fq.record(b"w%d" % i, fq.seq_of(rng, n), fq.seq_of(rng, n, alphabet)))
    return b"".join(out)


INPUTS = {
    "mixed": lambda: fq.mixed_reads(),
    "mixed_crlf": lambda: fq.mixed_reads(nl=b"\r\n"),
    "mixed_cr": lambda: fq.mixed_reads(nl=b"\r"),
    "mixed_no_final_newline": lambda: fq.mixed_reads()[:-1],
    "mixed_trailing_blank_lines": lambda: fq.mixed_reads() + b"\n\r\n\n\r\n\n",
    "spaces_and_tabs_in_sequence": lambda: b"@a\nAC GT\tA \n+\n!I5I4!I!\n@b\nAC\t\n+\n4!!\n@c\n\tA\n+\n!4\n",
    "tab_run_over_a_chunk_edge": lambda: b"@a\n" + b"A" * 50 + b"\t" * 30 + b"\n+\n" + b"!I" * 40 + b"\n@b\n"
                                         + b"C" * 50 + b"\t" * 30 + b"G\n+\n" + b"I4!" * 27 + b"\n",
    "header_at_tile_edge_16383": lambda: fq.header_at(TILE - 1),
    "header_at_tile_edge_16384": lambda: fq.header_at(TILE),
    "header_at_tile_edge_16385": lambda: fq.header_at(TILE + 1),
    "header_at_chunk_edge_63": lambda: fq.header_at(63),
    "header_at_chunk_edge_64": lambda: fq.header_at(64),
    "header_at_chunk_edge_65": lambda: fq.header_at(65),
    "header_at_chunk_edge_in_tile_1": lambda: fq.header_at(TILE + 64 * 7 + 1),
    "sequence_and_quality_tiles_apart": lambda: fq.mixed_reads(n_records=20) + _one_read(40_000)
                                                + fq.mixed_reads(5, 20),
    "single_100k_read": lambda: _one_read(100_000),
    "first_base_masked": _first_base_masked,
    "wide_quality_bytes": _wide_quality_bytes,
}


@functools.lru_cache(maxsize=None)
def _text(case: str) -> bytes:
    return INPUTS[case]()


@functools.lru_cache(maxsize=None)
def _expected(case: str, min_qual: int, offset: int):
    """(codes, rec_seq, names, n_masked) of the masked records, by the FASTA oracle."""
    import np_oracle

    fasta, n_masked = mask_fastq(_text(case), min_qual, offset)
    recs = np_oracle.parse_fasta(fasta)
    codes, rec_seq = np_oracle.codes_of(recs)
    codes.setflags(write=False)
    rec_seq.setflags(write=False)
    return codes, rec_seq, [np_oracle.record_name(t) for t, _ in recs], n_masked


def _check_masked(dev, case: str, min_qual: int, offset: int) -> None:
    from kman_amd import engine

    codes_ref, rec_seq_ref, names, n_masked = _expected(case, min_qual, offset)
    text = _text(case)
    p = engine.parse_fastq(dev, text, min_qual, offset)
    try:
        assert p.n_records == len(names)
        assert p.n_bases == len(codes_ref)
        got = dev.download(p.codes, p.n_bases + 64, np.uint8)
        np.testing.assert_array_equal(got[: p.n_bases], codes_ref)
        assert (got[p.n_bases:] == 4).all()
        np.testing.assert_array_equal(p.rec_seq, rec_seq_ref)
        assert p.names == names
        assert len(p.name_off) == p.n_records + 1 and p.names_blob == b"".join(p.names)
        assert (np.frombuffer(text, np.uint8)[p.rec_hdr.astype(np.int64)] == ord("@")).all()
        assert p.n_masked == n_masked
    finally:
        p.free()


@pytest.mark.parametrize("min_qual, offset", THRESHOLDS, ids=lambda v: str(v))
@pytest.mark.parametrize("case", sorted(INPUTS))
def test_masked_parse_matches_oracle(dev, case, min_qual, offset):
    _check_masked(dev, case, min_qual, offset)


def test_threshold_bytes_above_0x80(dev):
    """Offset 64 + Q93 = 157: the unsigned compare at a threshold past 0x80."""
    codes_plain = _expected("wide_quality_bytes", 0, 33)[0]
    codes, _, _, n_masked = _expected("wide_quality_bytes", 93, 64)
    assert 0 < n_masked < len(codes) and (codes != codes_plain).any()
    _check_masked(dev, "wide_quality_bytes", 93, 64)
    _check_masked(dev, "mixed", 93, 64)  # (every byte of '!'..'~' is below)


def test_first_masked_base_keeps_the_record_bit(dev):
    codes = _expected("first_base_masked", 20, 33)[0]
    rec_seq = _expected("first_base_masked", 20, 33)[1]
    assert (codes[rec_seq.astype(np.int64)] == 12).all()  # N | record start, on the CPU side
    _check_masked(dev, "first_base_masked", 20, 33)


def test_min_qual_zero_is_the_plain_parse(dev):
    from kman_amd import engine

    for case in ("mixed", "header_at_tile_edge_16385", "spaces_and_tabs_in_sequence"):
        text = _text(case)
        plain = engine.parse_fastq(dev, text)
        try:
            want = dev.download(plain.codes, plain.n_bases + 64, np.uint8)
            for p in (engine.parse_fastq(dev, text, 0, 64), engine.parse(dev, text, "fastq", 0),
                      engine.parse(dev, text, min_qual=0, phred_offset=33)):
                try:
                    assert p.n_masked == 0 and p.n_bases == plain.n_bases
                    np.testing.assert_array_equal(dev.download(p.codes, p.n_bases + 64, np.uint8), want)
                    np.testing.assert_array_equal(p.rec_seq, plain.rec_seq)
                finally:
                    p.free()
        finally:
            plain.free()


def test_abi_entry_directly(dev):
    """kman_parse_fastq_q with a NULL n_masked, threshold byte 0, and a
    threshold byte past 255 (KMAN_EINVAL)."""
    from ctypes import byref, c_uint64, c_void_p

    from kman_amd import _native as N

    L = N.lib()
    text = _text("mixed")
    n = len(text)
    d_text, codes = dev.alloc(n + 64), dev.alloc(n + 64)
    cap = n // 4 + 1
    d_hdr, d_seq = dev.alloc(8 * cap), dev.alloc(8 * cap)
    try:
        dev.upload(d_text, text)
        args = (dev.ctx, c_void_p(d_text.ptr), n, c_void_p(codes.ptr), c_void_p(d_hdr.ptr), c_void_p(d_seq.ptr), cap)
        info, masked = N.ParseInfo(), c_uint64(7)
        for qbyte, off, q in ((0, 33, 0), (33 + 20, 33, 20)):
            want, _, _, n_masked = _expected("mixed", q, off)
            N.check(dev.ctx, L.kman_parse_fastq_q(*args, byref(info), qbyte, None), "kman_parse_fastq_q")
            assert int(info.n_bases) == len(want)
            np.testing.assert_array_equal(dev.download(codes, len(want), np.uint8), want)
            N.check(dev.ctx, L.kman_parse_fastq_q(*args, byref(info), qbyte, byref(masked)), "kman_parse_fastq_q")
            assert masked.value == n_masked
            np.testing.assert_array_equal(dev.download(codes, len(want), np.uint8), want)
        assert L.kman_parse_fastq_q(*args, byref(info), 256, byref(masked)) == N.KMAN_EINVAL
        assert masked.value == 0 and int(info.n_bases) == 0
    finally:
        for b in (d_text, codes, d_hdr, d_seq):
            b.free()


# ------------------------------------------------------------------ all masked


def _reads_below_tilde(total: int, seed: int = 23) -> bytes:
    """short_reads-like input whose quality bytes are '!'..'}' only."""
    rng = np.random.default_rng(seed)
    qual = np.arange(ord("!"), ord("}") + 1, dtype=np.uint8)
    out = []
    for i, n in enumerate(rng.integers(25, 151, total // 190).tolist()):
        out.append(fq.record(b"am%d" % i, fq.seq_of(rng, n), fq.seq_of(rng, n, qual)))
    return b"".join(out)


def _cli(argv):
    from kman_amd.scripts.kmer import main

    main([str(a) for a in argv], standalone_mode=False)


def test_all_bases_masked(dev, tmp_path):
    from kman_amd import engine

    text = _reads_below_tilde(200_000)
    assert b"~" not in b"".join(fq.fastq_lines(text)[3::4])
    n_bases = sum(len(x) for x in fq.fastq_lines(text)[1::4])
    p = engine.parse_fastq(dev, text, 93)
    try:
        assert p.n_masked == p.n_bases == n_bases
        got = dev.download(p.codes, p.n_bases, np.uint8)
        assert ((got & 7) == 4).all()
        assert engine.count_kmers(p, 21, False) == 0
        km = engine.extract(p, 21, False, want_pos=True)
        try:
            assert km.n == 0
        finally:
            km.free()
    finally:
        p.free()
    src, out = tmp_path / "all.fq", tmp_path / "count.txt"
    src.write_bytes(text)
    _cli(["count", src, out, 21, "-q", 93])
    assert out.read_bytes() == b""


# -------------------------------------------------------- extraction after mask


@pytest.fixture(scope="module")
def reads(tmp_path_factory):
    """~300 KB of 25- to 150-base reads, and their masked FASTA at Q20 (offset
    33) and at Q10 (offset 64), with the oracle's records of the first."""
    import np_oracle

    d = tmp_path_factory.mktemp("qreads")
    text = fq.short_reads(300_000)
    fa20, n20 = mask_fastq(text, 20, 33)
    fa10, n10 = mask_fastq(text, 10, 64)
    (d / "reads.fq").write_bytes(text)
    (d / "q20.fa").write_bytes(fa20)
    (d / "q10_64.fa").write_bytes(fa10)
    with gzip.open(d / "reads.fq.gz", "wb", compresslevel=1) as fh:
        fh.write(text)
    return {"text": text, "recs20": np_oracle.parse_fasta(fa20), "n20": n20, "fq": str(d / "reads.fq"),
            "gz": str(d / "reads.fq.gz"), "q20": str(d / "q20.fa"), "q10_64": str(d / "q10_64.fa")}


@pytest.fixture(scope="module")
def parsed_q20(dev, reads):
    from kman_amd import engine

    p = engine.parse_fastq(dev, reads["text"], 20)
    yield p
    p.free()


@pytest.mark.parametrize("mode", ["fwd", "canon"])
@pytest.mark.parametrize("k", [5, 21, 32])
def test_extract_after_masking(dev, reads, parsed_q20, k, mode):
    import np_oracle
    from kman_amd import engine

    canon = mode == "canon"
    keys, pos = np_oracle.stream_kmers(reads["recs20"], k, canonical=canon)
    assert len(keys) > 0  # (the masked reads still hold k-mers at this k)
    assert parsed_q20.n_masked == reads["n20"]
    km = engine.extract(parsed_q20, k, False, want_pos=True, canonical=canon)
    try:
        assert km.n == len(keys)
        np.testing.assert_array_equal(dev.download(km.keys, km.n, np.uint64), keys)
        got_pos = dev.download(km.pos, km.n, np.uint32 if km.pos_bytes == 4 else np.uint64)
        np.testing.assert_array_equal(got_pos.astype(np.uint64), pos)
    finally:
        km.free()


# --------------------------------------------------------------------- errors

_GOOD = b"@a\nACGT\n+\nIIII\n@b\nAC\n+\nII\n@c\nACGTACGT\n+\nIIIIIIII\n"

ERRORS = {
    "no_at_in_record_3": (_GOOD.replace(b"@c", b"cc"), r"FASTQ record 3: header line does not start with '@'"),
    "no_plus_in_record_2": (_GOOD.replace(b"AC\n+\nII", b"AC\n-\nII"),
                            r"FASTQ record 2: separator line does not start with '\+'"),
    "short_quality_in_last_record": (_GOOD[:-2] + b"\n", r"FASTQ record 3: quality length 7 != sequence length 8"),
    "cut_after_1_line": (_GOOD + b"@d\n", r"FASTQ record 4: separator line does not start with '\+'"),
    "cut_after_2_lines": (_GOOD + b"@d\nACG\n", r"FASTQ record 4: separator line does not start with '\+'"),
    "cut_after_3_lines": (_GOOD + b"@d\nACG\n+\n", r"FASTQ record 4: quality length 0 != sequence length 3"),
    "empty_file": (b"", r"premature end of file or empty file"),
    "blank_lines": (b"\n\r\n\n\r", r"premature end of file or empty file"),
    "leading_blank_line": (b"\n" + _GOOD, r"FASTQ record 1: header line does not start with '@'"),
    "wrapped_fastq": (b"@a\nACGT\nACGT\n+\nIIII\nIIII\n", r"FASTQ record 1: separator line does not start with '\+'"),
    "first_of_many": (fq.mixed_reads(n_records=200) + b"@x\nACGT\n+\nIII\n" + fq.mixed_reads(3, 200) + b"oops\n",
                      r"FASTQ record 201: quality length 3 != sequence length 4"),
    "long_read_short_quality": (fq.record(b"l", b"ACGT" * 10_000, b"!" * 100) + _GOOD,
                                r"FASTQ record 1: quality length 100 != sequence length 40000"),
}


@pytest.mark.parametrize("case", sorted(ERRORS))
def test_errors_are_unchanged_under_a_threshold(dev, case):
    from kman_amd import engine

    text, msg = ERRORS[case]
    with pytest.raises(AssertionError, match=msg):  # the restatement agrees on the message
        mask_fastq(text, 30)
    with pytest.raises(AssertionError, match=msg):
        engine.parse_fastq(dev, text, 30)
    # the context is still usable
    p = engine.parse_fastq(dev, _GOOD, 40)  # ('I' is Q40)
    try:
        assert p.n_masked == 0 and p.n_bases == 14
    finally:
        p.free()
    p = engine.parse_fastq(dev, _GOOD, 41)
    try:
        assert p.n_masked == 14
        assert ((dev.download(p.codes, 14, np.uint8) & 7) == 4).all()
    finally:
        p.free()


# ------------------------------------------------------------------- commands


def _kmer(*argv):
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    for v in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "KMAN_DIST"):
        env.pop(v, None)
    subprocess.run([sys.executable, "-m", "kman_amd"] + [str(a) for a in argv], check=True, env=env, cwd=ROOT)


def _oracle(oracle_bin, *argv):
    subprocess.run([oracle_bin] + [str(a) for a in argv], check=True)


@pytest.mark.parametrize("cmd, flags, src, masked", [
    ("count", ["-q", 20], "fq", "q20"),
    ("uniq", ["-q", 20], "fq", "q20"),
    ("count", ["-q", 10, "--phred-offset", 64], "fq", "q10_64"),
    ("count", ["--min-qual", 20], "gz", "q20"),
], ids=["count_q20", "uniq_q20", "count_q10_offset64", "count_q20_gz"])
def test_command_matches_oracle(reads, oracle_bin, tmp_path, cmd, flags, src, masked):
    got, want = tmp_path / "got.txt", tmp_path / "want.txt"
    _kmer(cmd, reads[src], got, 21, *flags)
    _oracle(oracle_bin, cmd, reads[masked], want, 21)
    assert want.stat().st_size > 0 and got.read_bytes() == want.read_bytes()


def test_hist_command_matches_oracle(reads, oracle_bin, tmp_path):
    """The canonical spectrum == the tally of the oracle's `count -r` rows
    whose sequence is <= its reverse complement (odd k), on the masked FASTA."""
    _kmer("hist", reads["fq"], tmp_path / "h.txt", 21, "-q", 20)
    _oracle(oracle_bin, "count", reads["q20"], tmp_path / "c.txt", 21, "-r")
    comp = bytes.maketrans(b"ACGT", b"TGCA")
    tally = {}
    for line in (tmp_path / "c.txt").read_bytes().splitlines():
        s, c = line.split(b"\t")
        if s <= s.translate(comp)[::-1]:
            tally[int(c)] = tally.get(int(c), 0) + 1
    want = b"".join(b"%d\t%d\n" % (c, tally[c]) for c in sorted(tally))
    assert len(tally) >= 1 and (tmp_path / "h.txt").read_bytes() == want


def test_api_batcher_min_qual(dev, reads, oracle_bin, tmp_path):
    """FastaBatcher(min_qual=...).do on a FASTQ: the joined count equals the
    oracle's on the masked FASTA."""
    from kman_amd.batcher import FastaBatcher
    from kman_amd.join import KJoiner

    b = FastaBatcher(size=200_000, fmt="fastq", min_qual=20, device=dev)
    batches = b.do(reads["fq"], 21).collection
    assert b.source.parsed.n_masked == reads["n20"]
    out = tmp_path / "got.txt"
    KJoiner(KJoiner.MODE.SEQ_COUNT).join(batches, str(out))
    _oracle(oracle_bin, "count", reads["q20"], tmp_path / "want.txt", 21)
    assert (tmp_path / "want.txt").stat().st_size > 0 and out.read_bytes() == (tmp_path / "want.txt").read_bytes()
