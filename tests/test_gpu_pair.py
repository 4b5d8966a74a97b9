"""Read pairs on the GPU (`kmer screen` / `kmer classify --mate`,
`--interleaved`): kman_zip_records against the plain statement of its bytes
(tests/pair_cases.py) at the shapes where it can go wrong, then the pair-joint
numbers against the existing kernels run on the two inputs separately, and the
command line on tiny files.  Every output buffer is followed by sentinel bytes
that must come back unchanged; the inputs are compared after every call."""

from __future__ import annotations

from ctypes import c_void_p

import numpy as np
import pytest
from click.testing import CliRunner

import median_cases as mc
import pair_cases as pc
import reads_cases as rcs
import screen_cases as sc

pytestmark = pytest.mark.gpu

from kman_amd import _native as N  # noqa: E402

T = N.KMAN_ZIP_TILE
CAP = N.KMAN_ZIP_SEG_CAP
GUARD = 64  # sentinel bytes after the pad
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


def _zip(dev, lengths1, lengths2, seed=1):
    """kman_zip_records on mates of these lengths; the codes (with the pad) and
    the table, both checked against the statement."""
    c1, r1, n1 = pc.mate_codes(lengths1, seed)
    c2, r2, n2 = pc.mate_codes(lengths2, seed + 1000)
    R = len(r1)
    assert len(r2) == R
    pad = np.full(64, 4, np.uint8)
    host = [np.concatenate([c1, pad]), r1, np.concatenate([c2, pad]), r2]
    bufs = [_up(dev, a) for a in host]
    size = n1 + n2 + 64
    d_out = _up(dev, np.full(size + GUARD, SENT, np.uint8))
    d_rec = _up(dev, np.full(2 * R + 2, 0xA5A5A5A5A5A5A5A5, np.uint64))
    try:
        rc = N.lib().kman_zip_records(dev.ctx, c_void_p(bufs[0].ptr), n1, c_void_p(bufs[1].ptr), c_void_p(bufs[2].ptr),
                                      n2, c_void_p(bufs[3].ptr), R, c_void_p(d_out.ptr), c_void_p(d_rec.ptr))
        assert rc == N.KMAN_OK, N.lib().kman_last_error(dev.ctx)
        got = dev.download(d_out, size + GUARD, np.uint8)
        rec = dev.download(d_rec, 2 * R + 2, np.uint64)
        for a, b in zip(host, bufs):  # the inputs are never modified
            if a.nbytes:
                assert (dev.download(b, a.nbytes, np.uint8) == a.view(np.uint8)).all()
    finally:
        for b in bufs + [d_out, d_rec]:
            b.free()
    want, want_rec = pc.zip_codes(c1, r1, n1, c2, r2, n2)
    total = n1 + n2 if R else 0
    assert len(want) == total + 64
    assert (got[total + 64:] == SENT).all(), "bytes past the pad were written"
    assert (rec[2 * R:] == np.uint64(0xA5A5A5A5A5A5A5A5)).all(), "entries past the table were written"
    bad = np.nonzero(got[:total + 64] != want)[0]
    assert len(bad) == 0, "first differing byte %d of %d: %d for %d" % (bad[0], total, got[bad[0]], want[bad[0]])
    np.testing.assert_array_equal(rec[:2 * R], want_rec)
    return got[:total]


# ------------------------------------------------------------ kman_zip_records


@pytest.mark.parametrize("l1, l2", [([5], [7]), ([1], [1]), ([0], [3]), ([3], [0]), ([0], [0]), ([40], [1]),
                                    ([3 * T + 5], [2])])
def test_one_pair(dev, l1, l2):
    _zip(dev, l1, l2)


def test_degenerate_sizes(dev):
    _zip(dev, [], [])                          # no pairs: the pad alone
    _zip(dev, [0, 0, 0], [0, 0, 0])            # pairs without bases: zeros and the pad
    for l1, l2 in (([3, 2], [4, 1]), ([0, 15], [0, 0]), ([1, 1, 1], [1, 1, 1]), ([7], [8])):
        assert sum(l1) + sum(l2) < 16
        _zip(dev, l1, l2)                      # fewer than 16 bases in all: one partial word


def test_empty_mates_and_short_mates(dev):
    """A mate of 0 bases on either side and on both, among mates of 1, 15, 16
    and 17 bases in every order."""
    sizes = [0, 1, 15, 16, 17]
    l1 = [a for a in sizes for _ in sizes] * 2
    l2 = [b for _ in sizes for b in sizes] * 2
    l2[len(sizes) ** 2:] = l2[len(sizes) ** 2:][::-1]
    got = _zip(dev, l1, l2, seed=3)
    assert (0, 0) in zip(l1, l2) and (0, 17) in zip(l1, l2) and (17, 0) in zip(l1, l2)
    assert int(((got & 8) != 0).sum()) == sum(1 for x in l1 + l2 if x)  # bit 3: one per mate that has bases


def test_every_source_and_destination_alignment(dev):
    """Mates start at every residue mod 16 in both sources, each at every
    residue mod 16 of the output; some codes are masked (bit 2), bit 3 marks
    every start."""
    rng = np.random.default_rng(5)
    l1 = rng.integers(0, 40, 3000).tolist()
    l2 = rng.integers(0, 40, 3000).tolist()
    s1, s2 = np.cumsum([0] + l1[:-1]), np.cumsum([0] + l2[:-1])
    o1, o2 = s1 + s2, s1 + np.asarray(l1) + s2
    for src, out, ln in ((s1, o1, l1), (s2, o2, l2)):
        seen = {(int(a) % 16, int(b) % 16) for a, b, n in zip(src, out, ln) if n >= 17}
        assert len(seen) == 256
    got = _zip(dev, l1, l2, seed=7)
    assert (got & 4).any() and (got & 8).any()


@pytest.mark.parametrize("e", [-1, 0, 1])
def test_segments_at_the_tile_edges(dev, e):
    """A mate that ends one byte before, at and one byte after a tile edge; a
    mate over more than three tiles; a mate that starts in a tile's last byte."""
    l1 = [T + e - 9, 3 * T + 5, 7, 50]
    l2 = [9, 11, 0, 2]
    l2[2] = T - 1 - (sum(l1[:3]) + sum(l2[:2])) % T  # pair 3's mate 1 then starts in the last byte of a tile
    assert (l1[0] + l2[0]) == T + e and (sum(l1[:3]) + sum(l2[:3])) % T == T - 1
    _zip(dev, l1, l2, seed=11 + e)
    _zip(dev, l2, l1, seed=21 + e)  # the long mates in the second source


def test_more_segments_in_a_tile_than_the_lds_slice(dev):
    """1-base and empty mates: about 2T segments per tile, far more than CAP;
    then long mates again (the next tiles stage their slices in LDS)."""
    R = 3 * T
    l1 = [i % 2 for i in range(R)] + [2 * T + 3, 1]
    l2 = [(i // 2) % 2 for i in range(R)] + [5, T]
    assert R > 4 * CAP and sum(l1[:R]) + sum(l2[:R]) == R
    _zip(dev, l1, l2, seed=13)
    _zip(dev, [0] * R + [1], [0] * R + [1], seed=14)  # long rows of empty pairs before the only bases


# ------------------------------------------------------------------- engine


def _count_table(dev, records, k, canonical=False):
    from kman_amd import engine

    p = engine.parse(dev, sc.fasta(records))
    try:
        t = engine.join_groups(p, k, False, "count", canonical=canonical)
    finally:
        p.free()
    return t if t is not None else engine.empty_count(dev, k)


def _pair_records(k, seed=31, n=60):
    """(mates 1, mates 2, genome): mates cut from a genome with repeats, some
    unrelated, some empty or shorter than k, one pair whose junction spells a
    genome k-mer."""
    rng = np.random.default_rng(seed)
    unit, twice, once = sc.rand_seq(rng, 300), sc.rand_seq(rng, 300), sc.rand_seq(rng, 900)
    genome = unit + once + unit + twice + sc.rand_seq(rng, 600) + unit + twice  # k-mers with counts 1, 2 and 3
    # a pair whose joint median (2) is neither mate's: mate 1 is mostly once (1), mate 2 mostly unit (3)
    m1 = [("levels", once[100:160] + twice[50:100])]
    m2 = [("levels", unit[50:150] + twice[150:200])]
    for i in range(n):
        a = int(rng.integers(0, len(genome) - 400))
        la, lb = int(rng.integers(k, 160)), int(rng.integers(k, 160))
        x, y = genome[a:a + la], sc.revcomp(genome[a + 200:a + 200 + lb])
        kind = i % 10
        if kind == 3:
            x = sc.rand_seq(rng, la)              # mate 1 is not the genome's
        elif kind == 4:
            y = ""                                # an empty mate 2
        elif kind == 5:
            x = x[:k - 1]                         # no window in mate 1
        elif kind == 6:
            x, y = "", ""
        elif kind == 7:
            y = sc.with_n(y, [(5, 9)]) if len(y) > 12 else y
        m1.append(("p%d" % i, x))
        m2.append(("p%d" % i, y))
    # the junction: mate 1 ends with k - 1 bases and mate 2 starts with the bases that follow them in the genome
    m1.append(("junction", sc.rand_seq(rng, 30) + genome[1000:1000 + k - 1]))
    m2.append(("junction", genome[1000 + k - 1:1000 + k + 5] + sc.rand_seq(rng, 30)))
    return m1, m2, genome


@pytest.fixture(scope="module")
def paired(dev):
    """One zipped input shared by the engine tests: the views, the table, and
    the per-mate results of the existing kernels on the two inputs parsed
    separately (computed before the zip frees their codes)."""
    from kman_amd import engine

    k = 15
    m1, m2, genome = _pair_records(k)
    table = _count_table(dev, [("g", genome)], k, canonical=True)
    host = sc.table_of([("g", genome)], k, canonical=True)
    p1, p2 = engine.parse(dev, pc.fastq(m1, "/1")), engine.parse(dev, pc.fastq(m2, "/2"))
    alone = {}
    for key, p in (("1", p1), ("2", p2)):
        alone["stats" + key], _, runs = engine.screen_solid(p, table, True, 2)
        alone["span" + key] = engine.solid_spans(runs, k)
        alone["codes" + key] = p.dev.download(p.codes, p.n_bases, np.uint8)
        alone["rec" + key], alone["n" + key] = p.rec_seq.copy(), p.n_bases
    pm = engine.zip_pairs(p1, p2)
    pv = engine.pair_view(pm)
    yield dict(k=k, m1=m1, m2=m2, table=table, host=host, pm=pm, pv=pv, p1=p1, p2=p2, **alone)
    pv.free()
    pm.free()
    engine.free_result(table)


def test_zip_pairs_engine(dev, paired):
    from kman_amd import engine

    pm, pv, p1, p2 = paired["pm"], paired["pv"], paired["p1"], paired["p2"]
    R = len(paired["m1"])
    want, want_rec = pc.zip_codes(paired["codes1"], paired["rec1"], paired["n1"], paired["codes2"], paired["rec2"],
                                  paired["n2"])
    assert pm.n_records == 2 * R and pm.n_bases == paired["n1"] + paired["n2"] and pm.mates == (p1, p2)
    np.testing.assert_array_equal(pm.rec_seq, want_rec)
    np.testing.assert_array_equal(dev.download(pm.codes, pm.n_bases + 64, np.uint8), want)
    assert p1.codes.ptr is None and p2.codes.ptr is None  # the sources' codes are freed
    assert pv.n_records == R and pv.rec_seq.tolist() == want_rec[0::2].tolist()
    assert list(pv.names) == [(n + "/1").encode() for n, _ in paired["m1"]]
    assert isinstance(pv.codes, engine.BorrowedBuffer) and pv.codes.ptr == pm.codes.ptr
    engine.pair_view(pm).free()  # a view freed: the codes stay
    assert pm.codes.ptr is not None


def test_pair_statistics_are_the_sums_of_the_mates(paired):
    """screen() on the pair view against screen() on the two inputs parsed
    separately: no window spans the mates, none is lost."""
    from kman_amd import engine

    k, host = paired["k"], paired["host"]
    got = engine.screen(paired["pv"], paired["table"], True)
    np.testing.assert_array_equal(got, pc.pair_stats(paired["stats1"], paired["stats2"]))
    np.testing.assert_array_equal(got, pc.pair_stats(sc.stats(paired["m1"], k, host, True),
                                                     sc.stats(paired["m2"], k, host, True)))
    # the junction pair: its two mates laid end to end hold a genome k-mer that no mate holds
    (_, a), (_, b) = paired["m1"][-1], paired["m2"][-1]
    joined = sc.stats([("j", a + b)], k, host, True)[0]
    assert int(joined[1]) > int(got[-1][1]) and int(joined[0]) == int(got[-1][0]) + k - 1
    # the mate view counts per mate
    st = engine.screen(paired["pm"], paired["table"], True)
    np.testing.assert_array_equal(st[0::2], paired["stats1"])
    np.testing.assert_array_equal(st[1::2], paired["stats2"])


def test_joint_median_and_mate_spans(paired):
    from kman_amd import engine

    k, host, m1, m2 = paired["k"], paired["host"], paired["m1"], paired["m2"]
    stats, med, runs = engine.screen_pairs(paired["pm"], paired["pv"], paired["table"], True, median=True, min_count=2)
    np.testing.assert_array_equal(stats, pc.pair_stats(paired["stats1"], paired["stats2"]))
    want = pc.pair_medians(m1, m2, k, host, True)
    assert med.tolist() == want
    a, b = mc.medians(m1, k, host, True), mc.medians(m2, k, host, True)
    assert sum(1 for w, x, y in zip(want, a, b) if w != x and w != y) >= 1  # the joint median is nobody's own
    span = engine.solid_spans(runs, k)
    for j in (0, 1):  # each mate's stretch is that of its file screened alone
        np.testing.assert_array_equal(span[j][0::2], paired["span1"][j])
        np.testing.assert_array_equal(span[j][1::2], paired["span2"][j])
    assert (span[1] > span[0]).any()
    # without the options only the joint rows are computed
    st2, med2, runs2 = engine.screen_pairs(paired["pm"], paired["pv"], paired["table"], True)
    assert med2 is None and runs2 is None
    np.testing.assert_array_equal(st2, stats)
    # the formatter on real numbers
    keep = engine.screen_keep(stats, 1, median=med, span=engine.pair_min_span(span), min_solid_len=20)
    names = [n + "/1" for n, _ in m1]
    s1 = list(zip(span[0][0::2].tolist(), span[1][0::2].tolist()))
    s2 = list(zip(span[0][1::2].tolist(), span[1][1::2].tolist()))
    assert keep.tolist() == [int(x) for x in pc.pair_keep(stats, med, s1, s2, min_hits=1, min_solid_len=20)]
    assert 0 < keep.sum() < len(keep)
    assert engine.emit_screen_pairs(paired["pv"], stats, keep, median=med, span=span) == \
        pc.pair_lines(names, stats, med, s1, s2, keep)


def test_classify_planes_are_the_sums_of_the_mates(dev):
    from kman_amd import engine

    k = 11
    rng = np.random.default_rng(41)
    ga, gb = sc.rand_seq(rng, 2000), sc.rand_seq(rng, 2000)
    m1 = [("x%d" % i, ga[50 * i:50 * i + 60]) for i in range(20)]
    m2 = [("x%d" % i, sc.revcomp(gb[40 * i:40 * i + 90]) if i % 3 == 0 else ga[50 * i + 100:50 * i + 170])
          for i in range(20)]
    m1.append(("e", ""))
    m2.append(("e", gb[100:150]))
    tables = [_count_table(dev, [("a", ga)], k, True), _count_table(dev, [("b", gb)], k, True)]
    ct = engine.color_table(dev, tables)
    try:
        alone = []
        for recs in (m1, m2):
            p = engine.parse(dev, sc.fasta(recs))
            try:
                alone.append(engine.classify(p, ct, 2, True, planes=True))
            finally:
                p.free()
        pm = engine.zip_pairs(engine.parse(dev, sc.fasta(m1)), engine.parse(dev, sc.fasta(m2)))
        try:
            res = engine.classify(engine.pair_view(pm), ct, 2, True, planes=True)
        finally:
            pm.free()
    finally:
        engine.free_result(ct)
    np.testing.assert_array_equal(res[0], alone[0][0] + alone[1][0])   # windows
    np.testing.assert_array_equal(res[4], alone[0][4] + alone[1][4])   # hits per reference
    # pairs whose mate 1 alone is reference 0's and which the longer mate 2 turns to reference 1
    flipped = [i for i in range(len(m1)) if alone[0][1][i] == 0 and res[1][i] == 1]
    assert flipped and all(i % 3 == 0 for i in flipped)


# ------------------------------------------------------------------------ CLI


def _cli(*argv):
    from kman_amd.scripts.kmer import main

    r = CliRunner().invoke(main, [str(a) for a in argv], catch_exceptions=False)
    assert r.exit_code == 0, r.output


def _names_of(fastq_text):
    lines = fastq_text.split(b"\n")
    return [pc.pair_key(lines[i][1:].split(b" ")[0]) for i in range(0, len(lines) - 1, 4)]


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp("pairs")
    k = 15
    m1, m2, genome = _pair_records(k, seed=51, n=40)
    texts = {"r1.fq": pc.fastq(m1, "/1"), "r2.fq": pc.fastq(m2, "/2"), "il.fq": pc.interleave_fastq(m1, m2),
             "host.fa": sc.fasta([("host", genome)])}
    for name, text in texts.items():
        (d / name).write_bytes(text)
    return d, k, m1, m2, texts


def test_cli_mate_reads_out_in_step(files):
    d, k, m1, m2, texts = files
    out, f1, f2 = d / "a.tsv", d / "a.1.fq", d / "a.2.fq"
    _cli("screen", d / "r1.fq", d / "host.fa", out, k, "--canonical", "--mate", d / "r2.fq", "--min-frac", 0.5,
         "--median", "--reads-out", f1, "--reads-out2", f2)
    tsv = out.read_bytes()
    host = sc.table_of([("host", sc.fasta_records(texts["host.fa"])[0][1])], k, True)
    st = pc.pair_stats(sc.stats(m1, k, host, True), sc.stats(m2, k, host, True))
    med = pc.pair_medians(m1, m2, k, host, True)
    keep = pc.pair_keep(st, med, min_frac=0.5)
    assert 0 < sum(keep) < len(keep)
    assert tsv == pc.pair_lines([n + "/1" for n, _ in m1], st, med, kept=keep)
    # each output is the host cut of its own source, so record i of the two are mates
    for f, src in ((f1, "r1.fq"), (f2, "r2.fq")):
        assert f.read_bytes() == rcs.cut_whole(texts[src], rcs.fastq_offsets(texts[src]), keep)
    assert _names_of(f1.read_bytes()) == _names_of(f2.read_bytes()) == \
        [n.encode() for (n, _), kp in zip(m1, keep) if kp]
    # -v: the other pairs, whole
    _cli("screen", d / "r1.fq", d / "host.fa", out, k, "--canonical", "--mate", d / "r2.fq", "--min-frac", 0.5, "-v",
         "--reads-out", f1, "--reads-out2", f2)
    inv = [not x for x in keep]
    assert f2.read_bytes() == rcs.cut_whole(texts["r2.fq"], rcs.fastq_offsets(texts["r2.fq"]), inv)
    assert len(_names_of(f1.read_bytes())) == sum(inv)


def test_cli_interleaved_is_the_mate_run(files):
    d, k, m1, m2, texts = files
    a, b, fi = d / "b.tsv", d / "c.tsv", d / "c.il.fq"
    opts = ["--canonical", "--solid", 2, "--median", "--min-solid-len", 30]
    _cli("screen", d / "r1.fq", d / "host.fa", a, k, "--mate", d / "r2.fq", *opts)
    _cli("screen", d / "il.fq", d / "host.fa", b, k, "--interleaved", *opts, "--reads-out", fi)
    assert a.read_bytes() == b.read_bytes() and a.read_bytes().count(b"\n") > 0
    assert all(line.count(b"\t") == 8 for line in a.read_bytes().splitlines())
    kept = [line.split(b"\t")[0] for line in a.read_bytes().splitlines()]
    keep2 = np.repeat([(n + "/1").encode() in kept for n, _ in m1], 2)
    assert fi.read_bytes() == rcs.cut_whole(texts["il.fq"], rcs.fastq_offsets(texts["il.fq"]), keep2)


def test_cli_trim_leaves_a_pair_out_of_both_files(files):
    d, k, m1, m2, texts = files
    out, f1, f2 = d / "d.tsv", d / "d.1.fq", d / "d.2.fq"
    _cli("screen", d / "r1.fq", d / "host.fa", out, k, "--canonical", "--mate", d / "r2.fq", "--solid", 1,
         "--reads-out", f1, "--reads-out2", f2, "--trim")
    rows = [line.split(b"\t") for line in out.read_bytes().splitlines()]
    assert len(rows) == len(m1)  # every pair is listed
    span1 = [(int(r[4]), int(r[5])) for r in rows]
    span2 = [(int(r[6]), int(r[7])) for r in rows]
    both = [a[1] > a[0] and b[1] > b[0] for a, b in zip(span1, span2)]
    one_only = [(a[1] > a[0]) != (b[1] > b[0]) for a, b in zip(span1, span2)]
    assert any(one_only) and any(both)  # pairs with a stretch in one mate alone exist, and are left out of both
    for f, src, span in ((f1, "r1.fq", span1), (f2, "r2.fq", span2)):
        want = rcs.cut_trimmed(texts[src], rcs.fastq_offsets(texts[src]), [s for s, _ in span], [e for _, e in span],
                               both)
        assert f.read_bytes() == want
    assert _names_of(f1.read_bytes()) == _names_of(f2.read_bytes()) == \
        [n.encode() for (n, _), kp in zip(m1, both) if kp]


def test_cli_classify_pairs_in_step(files):
    d, k, m1, m2, texts = files
    rng = np.random.default_rng(61)
    (d / "other.fa").write_bytes(sc.fasta([("other", sc.rand_seq(rng, 1500))]))
    out, prefix = d / "e.tsv", d / "e"
    _cli("classify", d / "r1.fq", out, k, "--ref", d / "host.fa", "--ref", d / "other.fa", "--canonical", "--mate",
         d / "r2.fq", "--reads-out-prefix", prefix, "--summary", d / "e.sum")
    rows = [line.split(b"\t") for line in out.read_bytes().splitlines()]
    assert [r[0] for r in rows] == [(n + "/1").encode() for n, _ in m1]
    classes = {"host": b"host", "other": b"other", "ambiguous": b"?", "unassigned": b"-"}
    total = 0
    for cls, lab in classes.items():
        keep = [r[2] == lab for r in rows]
        t1, t2 = ((d / ("e.%s.%d.fq" % (cls, j))).read_bytes() for j in (1, 2))
        assert t1 == rcs.cut_whole(texts["r1.fq"], rcs.fastq_offsets(texts["r1.fq"]), keep)
        assert t2 == rcs.cut_whole(texts["r2.fq"], rcs.fastq_offsets(texts["r2.fq"]), keep)
        assert _names_of(t1) == _names_of(t2)
        total += sum(keep)
    assert total == len(m1) and sum(r[2] == b"host" for r in rows) > 0
    summary = (d / "e.sum").read_bytes().splitlines()
    assert int(summary[0].split(b"\t")[2]) == sum(r[2] == b"host" for r in rows)  # --summary counts pairs
    # interleaved: the same lines, one interleaved file per class
    out2 = d / "f.tsv"
    _cli("classify", d / "il.fq", out2, k, "--ref", d / "host.fa", "--ref", d / "other.fa", "--canonical",
         "--interleaved", "--reads-out-prefix", d / "f")
    assert out2.read_bytes() == out.read_bytes()
    keep2 = np.repeat([r[2] == b"host" for r in rows], 2)
    assert (d / "f.host.fq").read_bytes() == rcs.cut_whole(texts["il.fq"], rcs.fastq_offsets(texts["il.fq"]), keep2)


def test_cli_without_the_options_is_unchanged(files):
    """A run without --mate / --interleaved: the single reads' bytes, as the
    statement of the single reads' command gives them."""
    import solid_cases as so

    d, k, m1, m2, texts = files
    out = d / "g.tsv"
    host = sc.table_of([("host", sc.fasta_records(texts["host.fa"])[0][1])], k, True)
    recs = [(n + "/1", s) for n, s in m1]
    _cli("screen", d / "r1.fq", d / "host.fa", out, k, "--canonical")
    assert out.read_bytes() == sc.lines(recs, sc.stats(recs, k, host, True))
    _cli("screen", d / "r1.fq", d / "host.fa", out, k, "--canonical", "--median", "--solid", 2)
    st, med = sc.stats(recs, k, host, True), mc.medians(recs, k, host, True)
    assert out.read_bytes() == so.lines(recs, st, so.spans(so.runs_of(recs, k, host, 2, True), k), med)
