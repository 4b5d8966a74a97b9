"""FASTQ input on the GPU: kman_parse_fastq against the FASTA oracles run on
the converted records (fastq_cases.fastq_to_fasta), the extract kernels at
read density, the commands, the errors and the format override."""

from __future__ import annotations

import gzip
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

import fastq_cases as fq
from conftest import GOLDEN, ROOT

pytestmark = pytest.mark.gpu

TILE = 16384


@pytest.fixture(scope="module")
def dev():
    from kman_amd import engine

    return engine.default_device()


def _check_parse(dev, text: bytes) -> None:
    import np_oracle
    from kman_amd import engine

    recs = np_oracle.parse_fasta(fq.fastq_to_fasta(text))
    codes_ref, rec_seq_ref = np_oracle.codes_of(recs)
    p = engine.parse_fastq(dev, text)
    try:
        assert p.n_records == len(recs)
        assert p.n_bases == len(codes_ref)
        got = dev.download(p.codes, p.n_bases + 64, np.uint8)
        np.testing.assert_array_equal(got[: p.n_bases], codes_ref)
        assert (got[p.n_bases:] == 4).all()
        np.testing.assert_array_equal(p.rec_seq, rec_seq_ref)
        assert p.names == [np_oracle.record_name(t) for t, _ in recs]
        assert len(p.name_off) == p.n_records + 1 and p.names_blob == b"".join(p.names)
        assert (np.frombuffer(text, np.uint8)[p.rec_hdr.astype(np.int64)] == ord("@")).all()
        assert (np.diff(p.rec_hdr.astype(np.int64)) > 0).all()
    finally:
        p.free()


def _one_read(n: int, seed: int = 9) -> bytes:
    rng = np.random.default_rng(seed)
    return fq.record(b"big one", fq.seq_of(rng, n), fq.qual_of(rng, n))


SMALL = {
    "mixed": lambda: fq.mixed_reads(),
    "mixed_crlf": lambda: fq.mixed_reads(nl=b"\r\n"),
    "mixed_cr": lambda: fq.mixed_reads(nl=b"\r"),
    "mixed_no_final_newline": lambda: fq.mixed_reads()[:-1],
    "mixed_trailing_blank_lines": lambda: fq.mixed_reads() + b"\n\r\n\n\r\n\n",
    "mixed_second_seed": lambda: fq.mixed_reads(seed=11, n_records=350),
    "one_record": lambda: b"@r\nACGTN\n+\n!!!!!\n",
    "one_empty_record": lambda: b"@r\n\n+\n\n",
    "one_empty_record_cut": lambda: b"@r\n\n+",
    "spaces_and_tabs_in_sequence": lambda: b"@a\nAC GT\tA \n+\nIIIIIIII\n@b\nAC\t\n+\nIII\n@c\n\tA\n+\nII\n",
    "tab_run_over_a_chunk_edge": lambda: b"@a\n" + b"A" * 50 + b"\t" * 30 + b"\n+\n" + b"I" * 80 + b"\n@b\n"
                                         + b"C" * 50 + b"\t" * 30 + b"G\n+\n" + b"I" * 81 + b"\n",
    "header_at_tile_edge_16383": lambda: fq.header_at(TILE - 1),
    "header_at_tile_edge_16384": lambda: fq.header_at(TILE),
    "header_at_tile_edge_16385": lambda: fq.header_at(TILE + 1),
    "header_at_chunk_edge_63": lambda: fq.header_at(63),
    "header_at_chunk_edge_64": lambda: fq.header_at(64),
    "header_at_chunk_edge_65": lambda: fq.header_at(65),
    "header_at_chunk_edge_in_tile_1": lambda: fq.header_at(TILE + 64 * 7 + 1),
    "sequence_over_three_tiles": lambda: fq.mixed_reads(n_records=20) + _one_read(40_000) + fq.mixed_reads(5, 20),
    "single_100k_read": lambda: _one_read(100_000),
}


@pytest.mark.parametrize("case", sorted(SMALL))
def test_parse_matches_oracle(dev, case):
    _check_parse(dev, SMALL[case]())


def test_parse_two_level_scan(dev):
    """More than 1024 tiles: the tile scan crosses a block boundary."""
    text = fq.long_reads(17 << 20)
    assert len(text) > 1024 * TILE
    _check_parse(dev, text)


# ------------------------------------------------------- extraction at density


@pytest.fixture(scope="module")
def reads(tmp_path_factory):
    """One ~2 MB file of 25- to 150-base reads, its FASTA and oracle records."""
    import np_oracle

    d = tmp_path_factory.mktemp("reads")
    text = fq.short_reads()
    fasta = fq.fastq_to_fasta(text)
    (d / "reads.fq").write_bytes(text)
    (d / "reads.fa").write_bytes(fasta)
    with gzip.open(d / "reads.fq.gz", "wb", compresslevel=1) as fh:
        fh.write(text)
    return {"text": text, "fasta": fasta, "recs": np_oracle.parse_fasta(fasta), "dir": d,
            "fq": str(d / "reads.fq"), "fa": str(d / "reads.fa"), "gz": str(d / "reads.fq.gz")}


@pytest.fixture(scope="module")
def parsed_reads(dev, reads):
    from kman_amd import engine

    p = engine.parse_fastq(dev, reads["text"])
    yield p
    p.free()


@pytest.mark.parametrize("mode", ["fwd", "rc", "canon"])
@pytest.mark.parametrize("k", [5, 21, 31, 32])
def test_extract_at_read_density(dev, reads, parsed_reads, k, mode):
    """Every 64-byte chunk of codes holds a record start, many records are
    shorter than k: keys and pos of engine.extract against the oracle."""
    import np_oracle
    from kman_amd import engine

    rc, canon = mode == "rc", mode == "canon"
    keys, pos = np_oracle.stream_kmers(reads["recs"], k, rc=rc, canonical=canon)
    km = engine.extract(parsed_reads, k, rc, want_pos=True, canonical=canon)
    try:
        assert km.n == len(keys)
        np.testing.assert_array_equal(dev.download(km.keys, km.n, np.uint64), keys)
        got_pos = dev.download(km.pos, km.n, np.uint32 if km.pos_bytes == 4 else np.uint64)
        np.testing.assert_array_equal(got_pos.astype(np.uint64), pos)
    finally:
        km.free()


def test_extract_words_k33_at_read_density(dev, reads, parsed_reads):
    import np_oracle
    from kman_amd import engine

    k = 33
    codes, rec_seq = np_oracle.codes_of(reads["recs"])
    c = (codes & 7).astype(np.uint64)
    n = len(c)
    rec_id = np.searchsorted(rec_seq, np.arange(n), side="right")
    bad = np.concatenate([[0], np.cumsum(c > 3)])
    i = np.arange(n - k + 1)
    ok = (bad[i + k] == bad[i]) & (rec_id[i] == rec_id[i + k - 1])
    st = i[ok]
    lo = np.zeros(len(st), np.uint64)
    for j in range(32):
        lo = (lo << np.uint64(2)) | c[st + 1 + j]
    hi = c[st]
    w = engine.extract_words(parsed_reads, k, False, want_pos=True)
    try:
        assert w.n == len(st)
        rows = engine.download_words(dev, w.words, w.n, k, w.stride)
        np.testing.assert_array_equal(rows[:, 0], hi)
        np.testing.assert_array_equal(rows[:, 1], lo)
        np.testing.assert_array_equal(dev.download(w.pos, w.n, np.uint64), st.astype(np.uint64) << np.uint64(1))
    finally:
        w.free()


# ------------------------------------------------------------------- commands


def _kmer(*argv):
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    for v in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "KMAN_DIST"):
        env.pop(v, None)
    subprocess.run([sys.executable, "-m", "kman_amd"] + [str(a) for a in argv], check=True, env=env, cwd=ROOT)


def _oracle(oracle_bin, *argv):
    subprocess.run([oracle_bin] + [str(a) for a in argv], check=True)


@pytest.mark.parametrize("cmd, k, flags, src", [
    ("count", 21, [], "fq"),
    ("count", 5, ["-r"], "fq"),
    ("uniq", 21, [], "fq"),
    ("count", 21, [], "gz"),
], ids=["count_k21", "count_k5_r", "uniq_k21", "count_k21_gz"])
def test_command_matches_oracle(reads, oracle_bin, tmp_path, cmd, k, flags, src):
    got, want = tmp_path / "got.txt", tmp_path / "want.txt"
    _kmer(cmd, reads[src], got, k, *flags)
    _oracle(oracle_bin, cmd, reads["fa"], want, k, *flags)
    assert want.stat().st_size > 0 and got.read_bytes() == want.read_bytes()


def _batch_records(d):
    out = []
    for fn in sorted(os.listdir(d)):
        opener = gzip.open if fn.endswith(".gz") else open
        with opener(os.path.join(d, fn), "rb") as fh:
            lines = fh.read().split(b"\n")
        assert lines[-1] == b"" and len(lines) % 2 == 1
        out += list(zip(lines[0:-1:2], lines[1:-1:2]))
    return sorted(out)


def test_batch_command_matches_oracle(reads, oracle_bin, tmp_path):
    _kmer("batch", reads["fq"], tmp_path / "got", 13, "-b", 5000)
    _oracle(oracle_bin, "batch", reads["fa"], tmp_path / "want", 13, "-b", 5000)
    got, want = _batch_records(tmp_path / "got"), _batch_records(tmp_path / "want")
    assert len(want) > 100_000 and got == want


def test_hist_command_matches_oracle(reads, oracle_bin, tmp_path):
    """The canonical spectrum == the tally of the oracle's `count -r` rows
    whose sequence is <= its reverse complement (odd k)."""
    _kmer("hist", reads["fq"], tmp_path / "h.txt", 21)
    _oracle(oracle_bin, "count", reads["fa"], tmp_path / "c.txt", 21, "-r")
    comp = bytes.maketrans(b"ACGT", b"TGCA")
    tally = {}
    for line in (tmp_path / "c.txt").read_bytes().splitlines():
        s, c = line.split(b"\t")
        if s <= s.translate(comp)[::-1]:
            tally[int(c)] = tally.get(int(c), 0) + 1
    want = b"".join(b"%d\t%d\n" % (c, tally[c]) for c in sorted(tally))
    assert len(tally) >= 1 and (tmp_path / "h.txt").read_bytes() == want


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
}


@pytest.mark.parametrize("case", sorted(ERRORS))
def test_errors(dev, case):
    from kman_amd import engine

    text, msg = ERRORS[case]
    with pytest.raises(AssertionError, match=msg):  # the restatement agrees on the message
        fq.fastq_to_fasta(text)
    with pytest.raises(AssertionError, match=msg):
        engine.parse_fastq(dev, text)
    _check_parse(dev, _GOOD)  # the context is still usable


# ------------------------------------------------------------ format override


def _cli(argv):
    from kman_amd.scripts.kmer import main

    main([str(a) for a in argv], standalone_mode=False)


def test_format_override(reads, golden_inputs, tmp_path):
    out = tmp_path / "o.txt"
    # (no line of this FASTQ starts with '>': read as FASTA it has no record at all)
    plain = tmp_path / "plain.fq"
    plain.write_bytes(b"".join(fq.record(b"r%d" % i, b"ACGTACGTACGTACGTACGTACGT", b"I" * 24) for i in range(50)))
    with pytest.raises(AssertionError, match="premature end of file or empty file"):
        _cli(["count", plain, out, 21, "-f", "fasta"])
    _cli(["count", plain, out, 21])  # (auto: read as FASTQ)
    assert out.read_bytes() == b"ACGTACGTACGTACGTACGTA\t50\nCGTACGTACGTACGTACGTAC\t50\n" \
                               b"GTACGTACGTACGTACGTACG\t50\nTACGTACGTACGTACGTACGT\t50\n"
    out.unlink()
    with pytest.raises(AssertionError, match="FASTQ record 1: header line does not start with '@'"):
        _cli(["count", golden_inputs["messy1"], out, 21, "-f", "fastq"])
    assert not out.exists()


def _golden_cases():
    import json

    with open(os.path.join(GOLDEN, "manifest.json")) as fh:
        cases = json.load(fh)["cases"]
    return [cases[0], cases[len(cases) // 2], cases[-1]]


@pytest.mark.parametrize("case", _golden_cases(), ids=lambda c: c["name"])
def test_format_auto_keeps_golden_fasta(case, golden_inputs, tmp_path):
    for fmt in ("auto", "fasta"):
        out = tmp_path / ("%s.txt" % fmt)
        _cli([case["cmd"], golden_inputs[case["input"]], out, case["k"], "-f", fmt] + case["flags"])
        assert hashlib.sha256(out.read_bytes()).hexdigest() == case["sha256"]


def test_api_batcher_format(dev, reads, oracle_bin, tmp_path):
    """FastaBatcher(fmt=...).do on a FASTQ: the joined count equals the oracle's."""
    from kman_amd.batcher import FastaBatcher
    from kman_amd.join import KJoiner

    for fmt in ("auto", "fastq"):
        batches = FastaBatcher(size=200_000, fmt=fmt, device=dev).do(reads["fq"], 21).collection
        out = tmp_path / ("%s.txt" % fmt)
        KJoiner(KJoiner.MODE.SEQ_COUNT).join(batches, str(out))
        if fmt == "auto":
            _oracle(oracle_bin, "count", reads["fa"], tmp_path / "want.txt", 21)
        assert out.read_bytes() == (tmp_path / "want.txt").read_bytes()
    with pytest.raises(AssertionError):
        FastaBatcher(fmt="bam")
