"""Homopolymer-compressed k-mers on the GPU (`--hpc`): kman_hpc_records
against the plain statement of its bytes (tests/hpc_cases.py) at the shapes
where it can go wrong, engine.hpc on parsed inputs, and the command line: a
command run with --hpc on X writes what the same command writes on the
compressed text of X.  Every output buffer is followed by sentinels that must
come back unchanged."""

from __future__ import annotations

from ctypes import byref, c_uint64, c_void_p

import numpy as np
import pytest
from click.testing import CliRunner

import hpc_cases as hc
import median_cases as mc
import pair_cases as pc
import reads_cases as rcs
import screen_cases as sc
import solid_cases as so

pytestmark = pytest.mark.gpu

from kman_amd import _native as N  # noqa: E402

T = N.KMAN_HPC_TILE
GUARD = 64
SENT = 0xA5
SENT64 = 0xA5A5A5A5A5A5A5A5
A, C, G, T_, NN, F = 0, 1, 2, 3, 4, 8


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


def _hpc(dev, codes, rec_seq):
    """kman_hpc_records with and without d_orig: codes, pad, table and map
    against the statement, the sentinels and the inputs unchanged."""
    codes = np.ascontiguousarray(codes, dtype=np.uint8)
    rec_seq = np.ascontiguousarray(rec_seq, dtype=np.uint64)
    n, R = len(codes), len(rec_seq)
    want, want_rec, want_orig = hc.hpc_codes(codes, rec_seq)
    m = len(want)
    host = np.concatenate([codes, np.full(64, 4, np.uint8)])
    for with_map in (False, True):
        d_in, d_rs = _up(dev, host), _up(dev, rec_seq)
        d_out = _up(dev, np.full(n + 64 + GUARD, SENT, np.uint8))
        d_rec = _up(dev, np.full(R + 2, SENT64, np.uint64))
        d_orig = _up(dev, np.full(n + 2, SENT64, np.uint64))
        n_out = c_uint64(SENT64)
        try:
            rc = N.lib().kman_hpc_records(dev.ctx, c_void_p(d_in.ptr), n, c_void_p(d_rs.ptr), R, c_void_p(d_out.ptr),
                                          c_void_p(d_rec.ptr), c_void_p(d_orig.ptr) if with_map else None,
                                          byref(n_out))
            assert rc == N.KMAN_OK, N.lib().kman_last_error(dev.ctx)
            got = dev.download(d_out, n + 64 + GUARD, np.uint8)
            rec = dev.download(d_rec, R + 2, np.uint64)
            orig = dev.download(d_orig, n + 2, np.uint64)
            assert (dev.download(d_in, n + 64, np.uint8) == host).all()
            if R:
                assert (dev.download(d_rs, R, np.uint64) == rec_seq).all()
        finally:
            for b in (d_in, d_rs, d_out, d_rec, d_orig):
                b.free()
        assert n_out.value == m
        bad = np.nonzero(got[:m] != want)[0]
        assert len(bad) == 0, "first differing byte %d of %d: %d for %d" % (bad[0], m, got[bad[0]], want[bad[0]])
        assert (got[m:m + 64] == 4).all(), "the pad"
        assert (got[m + 64:] == SENT).all(), "bytes past the pad were written"
        np.testing.assert_array_equal(rec[:R], want_rec)
        assert (rec[R:] == np.uint64(SENT64)).all(), "entries past the table were written"
        if with_map:
            np.testing.assert_array_equal(orig[:m], want_orig)
            assert (orig[m:] == np.uint64(SENT64)).all(), "entries past the map were written"
        else:
            assert (orig == np.uint64(SENT64)).all(), "d_orig was NULL"
    return want


def _cycle(n):
    """n codes, every neighbour different; bit 3 on the first."""
    c = (np.arange(n) % 4).astype(np.uint8)
    if n:
        c[0] |= F
    return c


# ---------------------------------------------------------- kman_hpc_records


@pytest.mark.parametrize("n", [0, 1, 2, 15, 16, 17, T - 1, T, T + 1, 3 * T + 5])
def test_sizes(dev, n):
    _hpc(dev, hc.skewed_codes(n, seed=n + 1), [0])
    _hpc(dev, hc.skewed_codes(n, seed=n + 2), [0, n // 2, n])


def test_runs_at_the_tile_edges(dev):
    c = _cycle(2 * T + 40)
    c[T - 2] = A
    c[T - 1:T + 4] = G                 # a run that starts at the last byte of a tile
    c[T + 4] = A
    c[2 * T - 5:2 * T + 1] = C         # a run that ends at the first byte of the next tile
    c[2 * T + 1] = A
    out = _hpc(dev, c, [0])
    assert len(out) == len(c) - 4 - 5
    # the same runs at the edges of a wave's 2 KiB and of a lane's word
    c = _cycle(T)
    for e in (2048, 1024, 16, 4096 + 1024):
        c[e - 1:e + 2] = (c[e - 2] + 1) % 4
    _hpc(dev, c, [0])


def test_a_whole_tile_inside_one_run(dev):
    c = _cycle(3 * T + 50)
    c[5:5 + 2 * T + 3] = T_            # tile 1 keeps nothing
    c[4], c[5 + 2 * T + 3] = A, A
    out = _hpc(dev, c, [0, 5, T, T + 1, 2 * T, 3 * T])
    assert len(out) == len(c) - (2 * T + 2)


def test_nothing_is_dropped(dev):
    c = _cycle(2 * T + 19)
    assert len(_hpc(dev, c, [0, 7])) == len(c)


def test_records(dev):
    # the same base at the end of record r and at the start of record r + 1: both kept
    c = np.asarray([A | F, C, G, G, G | F, G, A, A | F, A | F, C], np.uint8)
    assert _hpc(dev, c, [0, 4, 7, 8]).tolist() == [A | F, C, G, G | F, A, A | F, A | F, C]
    # empty records at the front, in the middle and at the end
    c = hc.skewed_codes(300, 5, starts=(10, 50))
    _hpc(dev, c, [0, 0, 0, 10, 10, 10, 50, 300, 300])
    # a record that starts at a tile's first byte and one at its last byte, inside runs of its base
    c = hc.skewed_codes(2 * T + 100, 6, p=(0.85, 0.05, 0.05, 0.05), n_frac=0.0)
    c[T - 3:T + 3] = A
    c[2 * T - 4:2 * T + 2] = A
    c[T] |= F
    c[2 * T - 1] |= F
    out = _hpc(dev, c, [0, T, 2 * T - 1])
    assert int(((out & F) != 0).sum()) == 3
    # bases before rec_seq[0]
    c = np.asarray([G, G, G, C, C, A, A, A | F, A, T_, T_ | F, T_], np.uint8)
    assert _hpc(dev, c, [7, 10]).tolist() == [G, C, A, A | F, T_, T_ | F]


def test_not_acgt_is_kept(dev):
    c = np.asarray([A | F, NN, NN, NN, A, A, NN, NN, C], np.uint8)
    assert _hpc(dev, c, [0]).tolist() == [A | F, NN, NN, NN, A, NN, NN, C]
    # A N A with the N a masked base (bit 2 on the base's code): three bytes stay
    c = np.asarray([A | F, A | NN, A, A, C | NN, C | NN, C], np.uint8)
    assert _hpc(dev, c, [0]).tolist() == [A | F, A | NN, A, C | NN, C | NN, C]
    c = hc.skewed_codes(T + 33, 8, n_frac=0.4)
    _hpc(dev, c, [0])


def test_one_base_records(dev):
    R = 5000
    c = np.full(R, A | F, np.uint8)
    assert len(_hpc(dev, c, np.arange(R))) == R


def test_random_skewed(dev):
    n = 4 * T + 7
    rng = np.random.default_rng(9)
    starts = np.unique(np.concatenate([[0], rng.integers(0, n, 300)]))
    c = hc.skewed_codes(n, 10, starts=starts.tolist())
    out = _hpc(dev, c, starts)
    assert len(out) < 0.7 * n


def test_a_table_that_is_not_ascending(dev):
    c = hc.skewed_codes(T + 100, 11)
    _hpc(dev, c, [900, 3, 2 ** 63, T + 99, 0, 2 ** 64 - 1])  # every entry on its own, clamped


def test_einval_writes_nothing(dev):
    n, R = 100, 2
    d_in = _up(dev, np.concatenate([hc.skewed_codes(n, 12), np.full(64, 4, np.uint8)]))
    d_rs = _up(dev, np.asarray([0, 40], np.uint64))
    d_out = _up(dev, np.full(n + 64 + GUARD, SENT, np.uint8))
    d_rec = _up(dev, np.full(R + 2, SENT64, np.uint64))
    d_orig = _up(dev, np.full(n + 2, SENT64, np.uint64))
    before = dev.download(d_in, n + 64, np.uint8).copy()
    i, rs, o, rec, og = d_in.ptr, d_rs.ptr, d_out.ptr, d_rec.ptr, d_orig.ptr
    bad = [
        (None, rs, o, rec, og), (i, None, o, rec, og), (i, rs, None, rec, og), (i, rs, o, None, og),  # NULL
        (i + 1, rs, o, rec, og), (i, rs, o + 8, rec, og), (i, rs + 4, o, rec, og), (i, rs, o, rec + 4, og),
        (i, rs, o, rec, og + 4),                                                                      # misaligned
        (i, rs, i, rec, og), (i, rs, i + 16, rec, og),                                                # in place, overlapping
    ]
    try:
        for a in bad:
            n_out = c_uint64(7)
            rc = N.lib().kman_hpc_records(dev.ctx, c_void_p(a[0]), n, c_void_p(a[1]), R, c_void_p(a[2]),
                                          c_void_p(a[3]), c_void_p(a[4]), byref(n_out))
            assert rc == N.KMAN_EINVAL, a
        assert N.lib().kman_hpc_records(dev.ctx, c_void_p(i), n, c_void_p(rs), R, c_void_p(o), c_void_p(rec), None,
                                        None) == N.KMAN_EINVAL
        assert (dev.download(d_out, n + 64 + GUARD, np.uint8) == SENT).all()
        assert (dev.download(d_rec, R + 2, np.uint64) == np.uint64(SENT64)).all()
        assert (dev.download(d_orig, n + 2, np.uint64) == np.uint64(SENT64)).all()
        assert (dev.download(d_in, n + 64, np.uint8) == before).all()
    finally:
        for b in (d_in, d_rs, d_out, d_rec, d_orig):
            b.free()


# -------------------------------------------------------------------- engine


def _small_fasta():
    rng = np.random.default_rng(21)
    recs = [("multi", sc.rand_seq(rng, 700)), ("empty", ""), ("nrun", sc.with_n(sc.rand_seq(rng, 300), [(40, 47), (100, 101)])),
            ("lower", sc.rand_seq(rng, 120).lower()), ("runs", "AAAAACCCCCGGGGGTTTTT" * 6), ("one", "A"), ("tail", sc.rand_seq(rng, 61))]
    text = b""
    for name, seq in recs:
        text += b">" + name.encode() + b" d\n" + b"".join(seq[i:i + 60].encode() + b"\n" for i in range(0, len(seq), 60))
    return text, recs


def _check_engine_hpc(dev, p):
    from kman_amd import engine

    n, R = int(p.n_bases), int(p.n_records)
    codes0 = dev.download(p.codes, n, np.uint8).copy()
    rec0 = np.asarray(p.rec_seq, dtype=np.uint64).copy()
    names, hdr = [bytes(x) for x in p.names], np.asarray(p.rec_hdr).copy()
    want, want_rec, want_orig = hc.hpc_codes(codes0, rec0)
    ph = engine.hpc(p, keep_map=True)
    try:
        assert ph.n_bases == len(want) and ph.n_records == R
        got = dev.download(ph.codes, ph.n_bases + 64, np.uint8)
        assert (got[:ph.n_bases] == want).all() and (got[ph.n_bases:] == 4).all()
        np.testing.assert_array_equal(ph.rec_seq, want_rec)
        np.testing.assert_array_equal(dev.download(ph.hpc_orig, ph.n_bases, np.uint64), want_orig)
        np.testing.assert_array_equal(ph.hpc_rec_seq, rec0)
        assert ph.hpc_n_bases == n and [bytes(x) for x in ph.names] == names
        np.testing.assert_array_equal(ph.rec_hdr, hdr)
    finally:
        ph.free()
    return codes0


def test_engine_hpc_of_a_fasta(dev):
    from kman_amd import engine

    text, _ = _small_fasta()
    _check_engine_hpc(dev, engine.parse(dev, text))


def test_engine_hpc_of_a_masked_fastq(dev):
    """-q masks before the compression: a masked base inside a run splits it."""
    from kman_amd import engine

    seq = "AAAAAACCCCGGGGGGGTTTTACGT" * 8
    qual = "".join("#" if i % 7 == 3 else "I" for i in range(len(seq)))
    text = ("@q1\n%s\n+\n%s\n@q2\n%s\n+\n%s\n" % (seq, qual, seq[::-1], qual)).encode()
    p = engine.parse(dev, text, "fastq", 20, 33, keep_text=True)
    assert p.n_masked > 0
    codes0 = _check_engine_hpc(dev, p)
    masked = (codes0 & 4) != 0
    assert masked.any() and (masked[1:-1] & ((codes0[:-2] & 7) == (codes0[2:] & 7))).any()


@pytest.mark.parametrize("canonical", [False, True])
def test_counts_of_the_compressed_parse(dev, canonical):
    from kman_amd import engine

    text, _ = _small_fasta()
    rows = []
    for p in (engine.hpc(engine.parse(dev, text)), engine.parse(dev, hc.hpc_text(text))):
        try:
            r = engine.count_groups(p, 11, False, canonical)
            try:
                rows.append(engine.download_count(dev, r))
            finally:
                engine.free_result(r)
        finally:
            p.free()
    np.testing.assert_array_equal(rows[0][0], rows[1][0])
    np.testing.assert_array_equal(rows[0][1], rows[1][1])
    assert len(rows[0][0]) > 100


# ----------------------------------------------------------------------- CLI


def _cli(*argv):
    from kman_amd.scripts.kmer import main

    r = CliRunner().invoke(main, [str(a) for a in argv], catch_exceptions=False)
    assert r.exit_code == 0, r.output


K = 15   # the small inputs
KL = 21  # the long reads


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """Every input as X (d / name) and as the compressed text of X (d / "c" /
    name: the same file name, so `classify` derives the same label)."""
    d = tmp_path_factory.mktemp("hpc")
    rng = np.random.default_rng(41)
    text, _ = _small_fasta()
    genome = sc.rand_seq(rng, 3000)
    fq_text, fq_recs = rcs.planted_reads(seed=13)
    # pairs: mates of the genome, some with N, an empty mate, one shorter than k
    m1, m2 = [], []
    for i in range(24):
        a = int(rng.integers(0, len(genome) - 400))
        x, y = genome[a:a + int(rng.integers(K, 150))], sc.revcomp(genome[a + 200:a + 200 + int(rng.integers(K, 150))])
        if i % 6 == 2:
            y = ""
        elif i % 6 == 3:
            x = x[:K - 3]
        elif i % 6 == 4:
            x = sc.rand_seq(rng, 80)
        elif i % 6 == 5:
            y = sc.with_n(y, [(5, 9)])
        m1.append(("p%d" % i, x))
        m2.append(("p%d" % i, y))
    # long reads: 5 kb of one of two 20 kb references, the lengths of their homopolymer runs changed
    refs = {"refA": sc.rand_seq(rng, 20000), "refB": sc.rand_seq(rng, 20000)}
    long_reads, source = [], []
    for i in range(6):
        lab = "refA" if i % 2 == 0 else "refB"
        a = int(rng.integers(0, 15000))
        long_reads.append(("long%d" % i, hc.vary_homopolymers(refs[lab][a:a + 5000], rng)))
        source.append(lab)
    texts = {"small.fa": text, "genome.fa": sc.fasta([("g", genome)]), "reads.fq": fq_text,
             "r1.fq": pc.fastq(m1, "/1"), "r2.fq": pc.fastq(m2, "/2"), "long.fq": pc.fastq(long_reads),
             "refA.fa": sc.fasta([("refA", refs["refA"])]), "refB.fa": sc.fasta([("refB", refs["refB"])])}
    (d / "c").mkdir()
    for name, t in texts.items():
        (d / name).write_bytes(t)
        (d / "c" / name).write_bytes(hc.hpc_text(t))
    return d, texts, source


def _same(d, tag, cmd, inputs, tail, outs=("OUT",)):
    """`cmd inputs.. OUT k.. --hpc` against the command without --hpc on the
    compressed inputs: OUT and the files of `outs` named in `tail` ({tag}
    stands for the run) are byte-identical.  Returns the --hpc run's OUT."""
    res = []
    for run, comp in (("h", False), ("p", True)):
        argv = [cmd] + [(d / "c" / x if comp else d / x) for x in inputs]
        out = d / ("%s.%s.out" % (tag, run))
        argv.append(out)
        for a in tail:
            if isinstance(a, str) and a.startswith("IN:"):
                a = d / "c" / a[3:] if comp else d / a[3:]
            elif isinstance(a, str) and a.startswith("F:"):
                a = d / ("%s.%s.%s" % (tag, run, a[2:]))
            argv.append(a)
        _cli(*(argv + ([] if comp else ["--hpc"])))
        res.append([out.read_bytes()] + [(d / ("%s.%s.%s" % (tag, run, o))).read_bytes() for o in outs if o != "OUT"])
    assert res[0] == res[1]
    assert len(res[0][0]) > 0
    return res[0][0]


@pytest.mark.parametrize("x, k, opts", [("small.fa", K, []), ("small.fa", K, ["--canonical", "-L", 2]),
                                        ("long.fq", KL, []), ("reads.fq", 31, [])])
def test_cli_count(files, x, k, opts):
    d, _, _ = files
    _same(d, "count_%s_%d_%d" % (x, k, len(opts)), "count", [x], [k] + opts)


@pytest.mark.parametrize("x, k, opts", [("small.fa", K, []), ("long.fq", KL, ["--forward"])])
def test_cli_hist(files, x, k, opts):
    d, _, _ = files
    _same(d, "hist_%s" % x, "hist", [x], [k] + opts)


@pytest.mark.parametrize("op", ["intersect", "subtract", "union"])
def test_cli_sets(files, op):
    d, _, _ = files
    _same(d, "sets_" + op, "sets", ["reads.fq", "small.fa"] if op == "union" else ["long.fq", "refA.fa"],
          [KL if op != "union" else K, "--op", op, "--canonical"])


def test_cli_screen_plain_median_and_reads_out(files):
    d, texts, _ = files
    _same(d, "scr", "screen", ["reads.fq", "genome.fa"], [K, "--canonical"])
    _same(d, "scr_small", "screen", ["small.fa", "small.fa"], [K])
    out = _same(d, "scr_med", "screen", ["r1.fq", "genome.fa"], [K, "--canonical", "--median", "--min-frac", 0.5])
    # --reads-out: the ORIGINAL records of the listed reads
    ro = d / "scr_ro.fq"
    _cli("screen", d / "r1.fq", d / "genome.fa", d / "scr_ro.tsv", K, "--canonical", "--median", "--min-frac", 0.5,
         "--hpc", "--reads-out", ro)
    assert (d / "scr_ro.tsv").read_bytes() == out
    kept = {line.split(b"\t")[0] for line in out.splitlines()}
    names = [ln[1:] for ln in texts["r1.fq"].split(b"\n")[0::4] if ln]
    keep = [nm in kept for nm in names]
    assert 0 < sum(keep) < len(keep)
    assert ro.read_bytes() == rcs.cut_whole(texts["r1.fq"], rcs.fastq_offsets(texts["r1.fq"]), keep)


def test_cli_screen_mate(files):
    d, texts, _ = files
    out = _same(d, "mate", "screen", ["r1.fq", "genome.fa"], [K, "--canonical", "--mate", "IN:r2.fq", "--median"])
    assert out.count(b"\n") == 24
    f1, f2 = d / "mate.1.fq", d / "mate.2.fq"
    _cli("screen", d / "r1.fq", d / "genome.fa", d / "mate.tsv", K, "--canonical", "--mate", d / "r2.fq", "--hpc",
         "--min-frac", 0.9, "--reads-out", f1, "--reads-out2", f2)
    kept = {line.split(b"\t")[0] for line in (d / "mate.tsv").read_bytes().splitlines()}
    keep = [b"p%d/1" % i in kept for i in range(24)]
    assert 0 < sum(keep) < 24
    for f, src in ((f1, "r1.fq"), (f2, "r2.fq")):
        assert f.read_bytes() == rcs.cut_whole(texts[src], rcs.fastq_offsets(texts[src]), keep)


def test_cli_classify_long_reads(files):
    """The main property: with --hpc every long read goes to its source with
    all of its k-mers; without it the changed run lengths cost hits."""
    d, texts, source = files
    tail = [KL, "--ref", "IN:refA.fa", "--ref", "IN:refB.fa", "--canonical", "--hits", "--summary", "F:sum"]
    out = _same(d, "cls", "classify", ["long.fq"], tail, outs=("OUT", "sum"))
    rows = [line.split(b"\t") for line in out.splitlines()]
    assert [r[2].decode() for r in rows] == source
    assert all(int(r[3]) == int(r[1]) > 3000 and int(r[4]) < 10 for r in rows)  # every window hits the source
    # the statement agrees: the compressed read is the compressed stretch of its reference
    for (_, seq), lab in zip(hc.text_records(texts["long.fq"]), source):
        assert hc.hpc_seq(seq)[0] in hc.hpc_seq(hc.text_records(texts[lab + ".fa"])[0][1])[0]
    # without --hpc: fewer hits
    plain = d / "cls.plain.tsv"
    _cli("classify", d / "long.fq", plain, KL, "--ref", d / "refA.fa", "--ref", d / "refB.fa", "--canonical")
    prow = [line.split(b"\t") for line in plain.read_bytes().splitlines()]
    assert any(int(p[3]) < int(r[3]) for p, r in zip(prow, rows))
    # --reads-out-prefix: the original records of every class
    _cli("classify", d / "long.fq", d / "cls.ro.tsv", KL, "--ref", d / "refA.fa", "--ref", d / "refB.fa", "--canonical",
         "--hits", "--hpc", "--reads-out-prefix", d / "clsro")
    assert (d / "cls.ro.tsv").read_bytes() == out
    off = rcs.fastq_offsets(texts["long.fq"])
    for cls, lab in (("refA", "refA"), ("refB", "refB"), ("ambiguous", "?"), ("unassigned", "-")):
        keep = [r[2].decode() == lab for r in rows]
        assert (d / ("clsro.%s.fq" % cls)).read_bytes() == rcs.cut_whole(texts["long.fq"], off, keep)


def test_cli_classify_small_and_pairs(files):
    d, _, _ = files
    _same(d, "cls_small", "classify", ["reads.fq"], [K, "--ref", "IN:genome.fa", "--ref", "IN:small.fa", "--hits",
                                                     "--summary", "F:sum"], outs=("OUT", "sum"))
    _same(d, "cls_pair", "classify", ["r1.fq"], [K, "--ref", "IN:genome.fa", "--ref", "IN:small.fa", "--canonical",
                                                 "--mate", "IN:r2.fq"])


# ---------------------------------------------------------- screen --hpc --solid


def test_cli_screen_solid_in_original_columns(files):
    """START, END, --bed and --trim in the original record's columns: the spans
    of the compressed run (the statement of --solid on the compressed records)
    mapped by map_span."""
    d, texts, _ = files
    rng = np.random.default_rng(77)
    genome = hc.text_records(texts["genome.fa"])[0][1]

    def stretch_ending_in_a_run(lo):
        # b: genome[b - 2] == genome[b - 1] != genome[b], so a read cut at b ends its match with a run of two
        for b in range(lo, len(genome) - 1):
            if genome[b - 2] == genome[b - 1] != genome[b] and genome[b - 3] != genome[b - 1]:
                return b
        raise AssertionError("no run in the genome")

    b = stretch_ending_in_a_run(700)
    junk = [x for x in "ACGT" if x not in (genome[b - 1], genome[b])][0] + sc.rand_seq(rng, 39)
    recs = [
        ("whole", genome[100:260]),                                     # the stretch ends at the record's last base
        ("run_end", genome[b - 120:b] + junk),                          # .. at a run of two, junk after it
        ("head", sc.rand_seq(rng, 35) + genome[1500:1620]),             # START > 0
        ("varied", hc.vary_homopolymers(genome[2000:2200], rng)),       # other run lengths than the genome's
        ("both", sc.rand_seq(rng, 30) + hc.vary_homopolymers(genome[2500:2650], rng) + sc.rand_seq(rng, 30)),
        ("none", sc.rand_seq(rng, 90)), ("short", genome[5:5 + K - 4]), ("empty", ""),
    ]
    text = pc.fastq(recs)
    (d / "solid.fq").write_bytes(text)
    out, bed, ro = d / "solid.tsv", d / "solid.bed", d / "solid.trim.fq"
    _cli("screen", d / "solid.fq", d / "genome.fa", out, K, "--canonical", "--hpc", "--solid", 1, "--median", "--bed", bed,
         "--reads-out", ro, "--trim")
    comp = [(n, hc.hpc_seq(s)[0]) for n, s in recs]
    table = sc.table_of([("g", hc.hpc_seq(genome)[0])], K, True)
    st, med = sc.stats(comp, K, table, True), mc.medians(comp, K, table, True)
    span_c = so.spans(so.runs_of(comp, K, table, 1, True), K)
    span = [hc.map_span(s, e, hc.hpc_seq(seq)[1], len(seq)) for (s, e), (_, seq) in zip(span_c, recs)]
    by = dict(zip([n for n, _ in recs], span))
    # the properties this input was built for
    assert by["whole"] == (0, 160)
    s, e = by["run_end"]
    assert e == 120 and recs[1][1][e - 1] == recs[1][1][e - 2] and span_c[1][1] < len(comp[1][1])
    assert by["head"][0] >= 30 and by["varied"] == (0, len(recs[3][1])) and span_c[3] != by["varied"]
    assert by["none"] == by["short"] == by["empty"] == (0, 0)
    assert out.read_bytes() == so.lines(recs, st, span, med)
    assert bed.read_bytes() == so.bed(recs, span)
    starts, ends = [a for a, _ in span], [b_ for _, b_ in span]
    assert ro.read_bytes() == rcs.cut_trimmed(text, rcs.fastq_offsets(text), starts, ends)
    # --min-solid-len counts original bases: 160 keeps "whole" (160 original, fewer compressed)
    assert span_c[0][1] - span_c[0][0] < 160
    _cli("screen", d / "solid.fq", d / "genome.fa", out, K, "--canonical", "--hpc", "--solid", 1, "--min-solid-len", 160)
    keep = so.keep(st, span, min_solid_len=160)
    assert keep[0] and out.read_bytes() == so.lines(recs, st, span, None, kept=keep)


def test_engine_hpc_spans(dev):
    from kman_amd import engine

    text = b">a\nAAACCGGGGT\n>e\n>b\nACGTT\n>c\nGGGG\n"
    p = engine.hpc(engine.parse(dev, text), keep_map=True)
    try:
        assert p.rec_seq.tolist() == [0, 4, 4, 8]
        s, e = engine.hpc_spans(p, (np.asarray([1, 0, 1, 0], np.uint64), np.asarray([3, 0, 4, 1], np.uint64)))
        assert list(zip(s.tolist(), e.tolist())) == [(3, 9), (0, 0), (1, 5), (0, 4)]
        s, e = engine.hpc_spans(p, (np.zeros(4, np.uint64), np.zeros(4, np.uint64)))
        assert not s.any() and not e.any()
    finally:
        p.free()
