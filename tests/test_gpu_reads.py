"""`kmer screen --reads-out` / `--trim` on the GPU: kman_cut_records against the
plain-Python statement of its bytes (tests/reads_cases.py) at every source and
destination alignment, at the tile edges of the copy pass, with more segments
in a tile than its LDS slice holds, under sizing, capacity and slicing, trimmed
records, clamped offsets; then engine.cut_records on parsed FASTA and FASTQ and
the command line.  Every output buffer is followed by sentinel bytes that must
come back unchanged; the inputs are compared after every call."""

from __future__ import annotations

import ctypes
import gzip
from ctypes import byref, c_size_t, c_uint64, c_void_p

import numpy as np
import pytest
from click.testing import CliRunner

import fasta_cases as fc
import fastq_cases as fq
import reads_cases as rcs
import screen_cases as sc

pytestmark = pytest.mark.gpu

from kman_amd import _native as N  # noqa: E402

T = N.KMAN_CUT_TILE
CAP = N.KMAN_CUT_SEG_CAP
TRIM = N.KMAN_CUT_TRIM
PAD = 64  # sentinel bytes after an output
SENT = 0xA5


@pytest.fixture(scope="module")
def dev():
    from kman_amd import engine

    return engine.default_device()


def _up(dev, arr):
    arr = np.ascontiguousarray(arr)
    buf = dev.alloc(max(16, arr.nbytes))
    if arr.nbytes:
        dev.upload(buf, arr)
    return buf


def _plan(n_records, flags):
    need = c_uint64(0)
    assert N.lib().kman_cut_records_plan(n_records, flags, byref(need)) == N.KMAN_OK
    return need.value


class Cut:
    """One input on the device: text, offsets, keep and span arrays; call() runs
    kman_cut_records on a slice of the records and returns (rc, used, the
    output buffer's cap bytes); the sentinel bytes after cap and the inputs are
    checked on the way."""

    def __init__(self, dev, text, off, keep=None, start=None, end=None):
        self.dev, self.text = dev, bytes(text)
        self.host = [np.frombuffer(self.text, np.uint8), np.asarray(off, np.uint64),
                     None if keep is None else np.asarray(keep, np.uint8),
                     None if start is None else np.asarray(start, np.uint64),
                     None if end is None else np.asarray(end, np.uint64)]
        self.bufs = [None if a is None else _up(dev, a) for a in self.host]
        self.R = len(off) - 1

    def call(self, cap=None, flags=None, i0=0, m=None, out=True, work_bytes=None, n_bytes=None):
        dev, L = self.dev, N.lib()
        d_text, d_off, d_keep, d_start, d_end = self.bufs
        m = self.R - i0 if m is None else m
        flags = (TRIM if d_start is not None else 0) if flags is None else flags
        need = _plan(max(m, 1), flags & TRIM)
        work = dev.alloc(max(16, need))
        cap = 0 if cap is None else cap
        obuf = _up(dev, np.full(cap + PAD, SENT, np.uint8))
        used = c_size_t(12345)

        def at(b, nbytes):
            return c_void_p(b.ptr + nbytes) if b is not None else None

        try:
            rc = L.kman_cut_records(dev.ctx, c_void_p(d_text.ptr), len(self.text) if n_bytes is None else n_bytes,
                                    at(d_off, 8 * i0), m, at(d_keep, i0), at(d_start, 8 * i0), at(d_end, 8 * i0), flags,
                                    c_void_p(work.ptr), need if work_bytes is None else work_bytes,
                                    c_void_p(obuf.ptr) if out else None, cap, byref(used))
            got = dev.download(obuf, cap + PAD, np.uint8)
        finally:
            work.free()
            obuf.free()
        assert (got[cap:] == SENT).all(), "bytes at or past d_out + cap were written"
        for a, b in zip(self.host, self.bufs):  # the inputs are never modified
            if a is not None and a.nbytes:
                assert (dev.download(b, a.nbytes, np.uint8) == a.view(np.uint8)).all()
        return rc, used.value, got[:cap].tobytes()

    def free(self):
        for b in self.bufs:
            if b is not None:
                b.free()


def _want(text, off, keep=None, start=None, end=None):
    if start is None:
        return rcs.cut_whole(text, off, keep)
    return rcs.cut_trimmed(text, off, start, end, keep)


def _check(dev, text, off, keep=None, start=None, end=None):
    """sizing, then a call with exactly that capacity: the statement's bytes"""
    want = _want(text, off, keep, start, end)
    c = Cut(dev, text, off, keep, start, end)
    try:
        rc, used, _ = c.call(out=False)
        assert (rc, used) == (N.KMAN_ECAP if want else N.KMAN_OK, len(want))
        rc, used, got = c.call(cap=len(want))
        assert (rc, used) == (N.KMAN_OK, len(want))
        assert got == want
    finally:
        c.free()
    return want


# ------------------------------------------------------------------ alignment


def test_every_source_and_destination_alignment(dev):
    """Records of 1, 15, 16, 17 and 33 bytes at every (source offset mod 16,
    destination offset mod 16): before each, a written record moves the output
    position and an unlisted one the source position."""
    lengths, keep, pairs = [], [], set()
    src = out = 0
    for s in range(16):
        for d in range(16):
            for n in (1, 15, 16, 17, 33):
                p = (d - out) % 16          # written: moves both
                g = (s - (src + p)) % 16    # not written: moves the source alone
                lengths += [p, g, n]
                keep += [1, 0, 1]
                src, out = src + p + g, out + p
                assert src % 16 == s and out % 16 == d
                pairs.add((src % 16, out % 16, n))
                src, out = src + n, out + n
    assert len(pairs) == 256 * 5
    text, off = rcs.byte_records(lengths, seed=3)
    want = _check(dev, text, off, keep)
    assert len(want) == out


# ----------------------------------------------------------------- tile edges


@pytest.mark.parametrize("e", [-1, 0, 1])
def test_records_at_the_tile_edges(dev, e):
    """A record that ends one byte before, at and one byte after output byte T;
    a record of 3T + 5 bytes; a record that starts in the last byte of a tile."""
    lengths = [T + e, 3 * T + 5, 7]
    lengths.append(T - 1 - sum(lengths) % T)  # the next one starts in the last byte of a tile
    lengths += [50, 2]
    assert sum(lengths[:4]) % T == T - 1
    text, off = rcs.byte_records(lengths, seed=5 + e, first=3)
    _check(dev, text, off)
    # with an unlisted record in front: another source alignment
    _check(dev, text, off, [0] + [1] * (len(lengths) - 1))


# -------------------------------------------------------------- keep patterns


@pytest.mark.parametrize("pattern", ["all", "none", "alternate", "first", "last", "null"])
def test_more_segments_in_a_tile_than_the_lds_slice(dev, pattern):
    R = T
    assert R > 4 * CAP
    lengths = [1 + i % 2 for i in range(R)]
    text, off = rcs.byte_records(lengths, seed=7)
    keep = {"all": np.ones(R, np.uint8), "none": np.zeros(R, np.uint8), "alternate": (np.arange(R) % 2).astype(np.uint8),
            "first": np.eye(1, R, 0, dtype=np.uint8)[0], "last": np.eye(1, R, R - 1, dtype=np.uint8)[0],
            "null": None}[pattern]
    want = _check(dev, text, off, keep)
    assert len(want) == {"all": 3 * R // 2, "none": 0, "alternate": R, "first": 1, "last": 2, "null": 3 * R // 2}[pattern]


def test_long_rows_of_unlisted_records_between_listed_ones(dev):
    lengths = [40] + [3] * (3 * CAP) + [2 * T] + [0] * CAP + [5] * (2 * CAP) + [33]
    keep = [1] + [0] * (3 * CAP) + [1] + [1] * CAP + [0] * (2 * CAP) + [1]
    text, off = rcs.byte_records(lengths, seed=8)
    _check(dev, text, off, keep)


# ------------------------------------------------------- sizing, capacity, slices


def test_sizing_capacity_and_slices(dev):
    text = fq.mixed_reads(seed=2, n_records=120)
    off = rcs.fastq_offsets(text)
    R = len(off) - 1
    rng = np.random.default_rng(4)
    keep = rng.integers(0, 2, R).astype(np.uint8)
    want = rcs.cut_whole(text, off, keep)
    c = Cut(dev, text, off, keep)
    try:
        assert c.call(out=False)[:2] == (N.KMAN_ECAP, len(want))           # d_out == NULL sizes only
        rc, used, got = c.call(cap=len(want) - 1)
        assert (rc, used) == (N.KMAN_ECAP, len(want))
        assert got == bytes([SENT]) * (len(want) - 1)                       # nothing is written at all
        rc, used, got = c.call(cap=len(want) + 100)
        assert (rc, used) == (N.KMAN_OK, len(want)) and got[:used] == want
        assert got[used:] == bytes([SENT]) * 100
        for cut in (1, 37, R - 1):                                          # two slices concatenate to the whole
            a = c.call(cap=len(want), i0=0, m=cut)
            b = c.call(cap=len(want), i0=cut, m=R - cut)
            assert a[0] == b[0] == N.KMAN_OK
            assert a[2][:a[1]] + b[2][:b[1]] == want
            assert a[2][:a[1]] == rcs.cut_whole(text, off[:cut + 1], keep[:cut])
        assert c.call(cap=64, m=0)[:2] == (N.KMAN_OK, 0)                    # no records: nothing is launched
    finally:
        c.free()


def test_refusals_write_nothing(dev):
    text = fq.mixed_reads(seed=2, n_records=20)
    off = rcs.fastq_offsets(text)
    R = len(off) - 1
    z = np.zeros(R, np.uint64)
    whole, trim = Cut(dev, text, off), Cut(dev, text, off, None, z, z + 5)
    try:
        size = len(text)
        for c, kw in ((whole, dict(flags=2)), (whole, dict(flags=TRIM)), (trim, dict(flags=0)),
                      (trim, dict(flags=TRIM | 4))):
            rc, used, got = c.call(cap=size, **kw)
            assert (rc, used) == (N.KMAN_EINVAL, 0) and got == bytes([SENT]) * size, kw
        rc, used, got = whole.call(cap=size, work_bytes=_plan(R, 0) - 16)
        assert (rc, used) == (N.KMAN_ECAP, 0) and got == bytes([SENT]) * size
        rc, used, got = trim.call(cap=size, work_bytes=_plan(R, 0))         # the plan of a whole cut is too small
        assert (rc, used) == (N.KMAN_ECAP, 0) and got == bytes([SENT]) * size
        L, u = N.lib(), c_size_t(7)
        d_text, d_off = whole.bufs[0], whole.bufs[1]
        work = dev.alloc(_plan(R, 0))
        try:
            args = lambda t, o, w: (dev.ctx, t, size, o, R, None, None, None, 0, w, _plan(R, 0), None, 0, byref(u))  # noqa: E731
            assert L.kman_cut_records(*args(None, c_void_p(d_off.ptr), c_void_p(work.ptr))) == N.KMAN_EINVAL
            assert L.kman_cut_records(*args(c_void_p(d_text.ptr), None, c_void_p(work.ptr))) == N.KMAN_EINVAL
            assert L.kman_cut_records(*args(c_void_p(d_text.ptr), c_void_p(d_off.ptr), None)) == N.KMAN_EINVAL
            assert L.kman_cut_records(*args(c_void_p(d_text.ptr + 8), c_void_p(d_off.ptr),
                                            c_void_p(work.ptr))) == N.KMAN_EINVAL
            assert u.value == 0
        finally:
            work.free()
    finally:
        whole.free()
        trim.free()


# ----------------------------------------------------------------------- trim


@pytest.mark.parametrize("i", range(len(rcs.HAND_TRIM)))
def test_trim_hand_cases(dev, i):
    rec, s, e, want = rcs.HAND_TRIM[i]
    assert _check(dev, rec, [0, len(rec)], None, [s], [e]) == want


def test_trim_hand_cases_in_one_text(dev):
    cases = [c for c in rcs.HAND_TRIM if c[0][-1:] in (b"\n", b"\r")] + [rcs.HAND_TRIM[-1]]
    text = b"".join(c[0] for c in cases)
    off = np.cumsum([0] + [len(c[0]) for c in cases])
    for keep in (None, [i % 3 != 1 for i in range(len(cases))]):
        want = _check(dev, text, off, keep, [c[1] for c in cases], [c[2] for c in cases])
        assert want == b"".join(c[3] for i, c in enumerate(cases) if keep is None or keep[i])


def _random_spans(rng, text, off):
    """valid (START, END) per record, with START == END, END beyond the kept
    bytes and whole reads among them"""
    start, end = [], []
    for r in range(len(off) - 1):
        n = len(rcs.cols_of(rcs.record_lines(rcs.record_bytes(text, off, r))[1]))
        a = int(rng.integers(0, n + 1))
        b = int(rng.integers(a, n + 1))
        kind = r % 7
        if kind == 3:
            b = a                      # nothing is written
        elif kind == 4:
            b = n + 1 + r              # clamped
        elif kind == 5:
            a, b = 0, n                # the whole read
        start.append(a)
        end.append(b)
    return start, end


@pytest.mark.parametrize("nl", [b"\n", b"\r\n"])
def test_trim_mixed_reads(dev, nl):
    text = fq.mixed_reads(seed=6, n_records=300, nl=nl)
    off = rcs.fastq_offsets(text)
    rng = np.random.default_rng(12)
    start, end = _random_spans(rng, text, off)
    keep = (rng.integers(0, 4, len(off) - 1) != 0).astype(np.uint8)
    want = _check(dev, text, off, keep, start, end)
    assert want.count(b"\n") % 4 == 0 and b"\r" not in want and len(want) > 4000
    _check(dev, text, off, None, start, end)
    assert any(not rcs.record_lines(rcs.record_bytes(text, off, r))[1] for r in range(len(off) - 1))  # an empty L2


def test_trim_a_long_read_over_several_wave_steps(dev):
    rng = np.random.default_rng(13)
    n = 20_000
    long_ = fq.record(b"long one", fq.seq_of(rng, n), fq.qual_of(rng, n))
    short = [fq.record(b"s%d" % i, fq.seq_of(rng, 40 + i), fq.qual_of(rng, 40 + i)) for i in range(4)]
    text = short[0] + short[1] + long_ + short[2] + short[3][:-1]  # (no final newline)
    off = rcs.fastq_offsets(text)
    for a, b in ((1500, 18_000), (0, n), (1023, 1025), (n - 1, n), (5000, 5001)):
        want = _check(dev, text, off, None, [3, 0, a, 5, 10], [30, 41, b, 6, 43])
        assert len(want.split(b"\n")[9]) == b - a


def test_trim_blanks_inside_a_long_line(dev):
    """columns and codes part ways: blanks inside the sequence line, over more than one wave step"""
    rng = np.random.default_rng(14)
    seq = bytearray(fq.seq_of(rng, 3000))
    for at in rng.integers(0, 3000, 200).tolist():
        seq[at] = 0x20
    seq = bytes(seq) + b" \t "
    rec = fq.record(b"blanks", seq, fq.qual_of(rng, len(seq)))
    ncols = len(rcs.cols_of(seq))
    assert 2700 < ncols < 3000
    for a, b in ((0, ncols), (100, 2600), (ncols - 1, ncols + 9), (ncols, ncols + 1)):
        _check(dev, rec + rec, [0, len(rec), 2 * len(rec)], None, [a, 7], [b, 9])


# ------------------------------------------------------------------- clamping


def test_offsets_past_the_text_and_descending_pairs_are_clamped(dev):
    text = fq.mixed_reads(seed=15, n_records=40)
    n = len(text)
    good = rcs.fastq_offsets(text)
    off = good[:10] + [good[12], good[11], good[13], n + 100, n + 5, n, n - 30]  # descending pairs, past the end
    want = _check(dev, text, off)
    assert want == rcs.cut_whole(text, off) and len(want) > 100
    R = len(off) - 1
    _check(dev, text, off, None, [1] * R, [30] * R)
    # a text shorter than the offsets say (n_bytes clamps them all)
    c = Cut(dev, text, good)
    try:
        short = n // 3
        w = rcs.cut_whole(text[:short], good)
        rc, used, got = c.call(cap=len(w), n_bytes=short)
        assert (rc, used, got) == (N.KMAN_OK, len(w), w)
    finally:
        c.free()


# --------------------------------------------------------------------- engine


def _fasta_texts():
    small = fc.small_cases()
    seen, out = set(), []
    for name, (text, meta) in small.items():
        if meta["family"] not in seen:
            seen.add(meta["family"])
            out.append((name, text))
    return out


def test_engine_cut_records_fasta(dev):
    from kman_amd import engine

    texts = _fasta_texts()
    assert len(texts) >= 5
    for name, text in texts:
        p = engine.parse(dev, text, keep_text=True)
        try:
            off = fc.header_offsets(text).tolist() + [len(text)]
            assert p.text is not None and p.text_bytes == len(text) and p.n_records == len(off) - 1
            assert bytes(engine.cut_records(p, None)) == rcs.cut_whole(text, off) == text[off[0]:], name
            keep = (np.arange(p.n_records) % 2 == 0).astype(np.uint8)
            assert bytes(engine.cut_records(p, keep)) == rcs.cut_whole(text, off, keep), name
        finally:
            p.free()
        assert p.text is None
    p = engine.parse(dev, texts[0][1])
    try:
        assert p.text is None and p.text_bytes == 0
        with pytest.raises(AssertionError, match="keep_text"):
            engine.cut_records(p, None)
    finally:
        p.free()


def test_engine_cut_records_fastq_in_slices(dev, tmp_path, monkeypatch):
    from kman_amd import engine

    rng = np.random.default_rng(16)
    big = fq.record(b"big", fq.seq_of(rng, 9000), fq.qual_of(rng, 9000))
    text = fq.mixed_reads(seed=17, n_records=80) + big + fq.mixed_reads(seed=18, n_records=30, nl=b"\r\n")
    off = rcs.fastq_offsets(text)
    R = len(off) - 1
    start, end = _random_spans(rng, text, off)
    keep = (rng.integers(0, 3, R) != 0).astype(np.uint8)
    path = tmp_path / "reads.fq"
    path.write_bytes(text)
    for slice_bytes in (None, 4096):  # (4096: several slices, the big read in a slice of its own)
        if slice_bytes:
            monkeypatch.setattr(engine.device, "_FMT_SLICE", slice_bytes)
        for p in (engine.parse(dev, text, keep_text=True), engine.parse_file(dev, str(path), keep_text=True)):
            try:
                assert p.n_records == R and p.rec_hdr.tolist() == off[:-1]
                assert bytes(engine.cut_records(p, None)) == text
                assert bytes(engine.cut_records(p, keep)) == rcs.cut_whole(text, off, keep)
                span = (np.array(start, np.uint64), np.array(end, np.uint64))
                want = rcs.cut_trimmed(text, off, start, end, keep)
                assert bytes(engine.cut_records(p, keep, span=span, trim=True)) == want
                with open(tmp_path / "out.fq", "wb") as fh:
                    fh.write(b"head\n")
                    assert engine.emit_reads(p, keep, fh, span=span, trim=True) is None
                    fh.write(b"tail\n")
                assert (tmp_path / "out.fq").read_bytes() == b"head\n" + want + b"tail\n"
            finally:
                p.free()
    p = engine.parse_file(dev, str(path))
    try:
        assert p.text is None
    finally:
        p.free()


# ------------------------------------------------------------------------ CLI


def _cli(*argv):
    from kman_amd.scripts.kmer import main

    r = CliRunner().invoke(main, [str(a) for a in argv], catch_exceptions=False)
    assert r.exit_code == 0, r.output


def _fastq_of(records, rng, nl=b"\n"):
    return b"".join(fq.record(name.encode() + b" d=%d" % i, seq.encode(), fq.qual_of(rng, len(seq)), nl=nl)
                    for i, (name, seq) in enumerate(records))


def test_cli_filtered_reads(tmp_path):
    """`--min-frac 0.5 -v --reads-out`: the reads that are not the host's, byte for byte."""
    k = 21
    rng = np.random.default_rng(19)
    host = sc.rand_seq(rng, 3000)
    recs = []
    for i in range(40):
        if i % 3 == 0:
            recs.append(("other%d" % i, sc.rand_seq(rng, 80 + i)))
        else:
            at = int(rng.integers(0, 3000 - 150))
            recs.append(("host%d" % i, host[at:at + 100 + i]))
    text = _fastq_of(recs, rng)[:-1]  # (the last read without a final newline)
    (tmp_path / "reads.fq").write_bytes(text)
    with gzip.open(tmp_path / "reads.fq.gz", "wb") as fh:
        fh.write(text)
    (tmp_path / "host.fa").write_bytes(sc.fasta([("host", host)]))
    off = rcs.fastq_offsets(text)
    out, clean = tmp_path / "clean.tsv", tmp_path / "clean.fq"
    for reads in ("reads.fq", "reads.fq.gz"):
        _cli("screen", tmp_path / reads, tmp_path / "host.fa", out, k, "--canonical", "--min-frac", 0.5, "-v",
             "--reads-out", clean)
        tsv = out.read_bytes()
        rows = [line.split(b"\t")[0].decode() for line in tsv.splitlines()]
        assert rows == [name for name, _ in recs if name.startswith("other")]
        keep = [name in rows for name, _ in recs]
        assert clean.read_bytes() == rcs.cut_whole(text, off, keep)
        # the TSV is that of the same command without the option
        _cli("screen", tmp_path / reads, tmp_path / "host.fa", out, k, "--canonical", "--min-frac", 0.5, "-v")
        assert out.read_bytes() == tsv
        clean.unlink()
    # fasta READS, every record listed: the input from its first header on
    fa = b"; a comment line\n" + sc.fasta(recs[:7])
    (tmp_path / "reads.fa").write_bytes(fa)
    _cli("screen", tmp_path / "reads.fa", tmp_path / "host.fa", out, k, "--reads-out", clean)
    assert clean.read_bytes() == fa[fa.index(b">"):]


def test_cli_trimmed_reads(tmp_path):
    """`--solid 2 --trim --bed` on self-screened reads with planted errors."""
    k = 15
    text, recs = rcs.planted_reads()
    (tmp_path / "reads.fq").write_bytes(text)
    off = rcs.fastq_offsets(text)
    out, bed, trimmed = tmp_path / "trim.tsv", tmp_path / "trim.bed", tmp_path / "trimmed.fq"
    _cli("screen", tmp_path / "reads.fq", tmp_path / "reads.fq", out, k, "--canonical", "--solid", 2, "--bed", bed)
    tsv0, bed0 = out.read_bytes(), bed.read_bytes()
    _cli("screen", tmp_path / "reads.fq", tmp_path / "reads.fq", out, k, "--canonical", "--solid", 2, "--bed", bed,
         "--reads-out", trimmed, "--trim")
    assert (out.read_bytes(), bed.read_bytes()) == (tsv0, bed0)  # unchanged by the options
    spans = {}
    for line in bed0.splitlines():
        name, a, b = line.split(b"\t")
        spans[name.decode()] = (int(a), int(b))
    seqs = dict(recs)
    assert 0 < len(spans) <= len(recs)
    assert any(b - a < len(seqs[n]) for n, (a, b) in spans.items())  # some read is really cut
    lines = trimmed.read_bytes().split(b"\n")
    assert lines[-1] == b"" and len(lines) == 4 * len(spans) + 1
    written = []
    for i in range(0, len(lines) - 1, 4):
        name = lines[i][1:].split(b" ")[0].decode()
        a, b = spans[name]
        assert lines[i + 1].decode() == seqs[name][a:b]
        assert lines[i + 2] == b"+" and len(lines[i + 3]) == b - a
        written.append(name)
    assert written == [n for n, _ in recs if n in spans]  # input order; reads absent from the BED are absent
    start = [spans.get(n, (0, 0))[0] for n, _ in recs]
    end = [spans.get(n, (0, 0))[1] for n, _ in recs]
    assert trimmed.read_bytes() == rcs.cut_trimmed(text, off, start, end)
    # whole reads of the same listing
    _cli("screen", tmp_path / "reads.fq", tmp_path / "reads.fq", out, k, "--canonical", "--solid", 2,
         "--min-solid-len", 40, "--reads-out", trimmed)
    rows = [line.split(b"\t")[0].decode() for line in out.read_bytes().splitlines()]
    assert 0 < len(rows) < len(recs)
    assert trimmed.read_bytes() == rcs.cut_whole(text, off, [n in rows for n, _ in recs])
