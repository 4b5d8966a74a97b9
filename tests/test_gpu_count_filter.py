"""The abundance filter on the GPU: kman_filter_counts against numpy, `kmer
count -L/-U` pinned to the reference's own output lines (tests/golden) and to
the oracles, `count --canonical` pinned to the reference's -r rows, and the
filter under simulated ranks."""

from __future__ import annotations

import functools
import os
import subprocess
import sys
from ctypes import byref, c_uint64, c_void_p

import numpy as np
import pytest

from conftest import GOLDEN, ROOT

pytestmark = pytest.mark.gpu

from kman_amd import _native as N  # noqa: E402

T = N.KMAN_FILTER_TILE
SIZES = [0, 1, T - 1, T, T + 1, 3 * T + 17, (1 << 20) + 3]  # the last: a look-back chain of 257 tiles
PATTERNS = ["all", "none", "alternating", "first_row", "last_row", "last_tile", "not_first_tile", "random"]
MIXED = {"alternating", "random"}  # (kept and dropped rows both exist once n >= 2 / a few rows)
PAD = 64  # sentinel rows after every device array
B32 = 1 << 32
_RC = bytes.maketrans(b"ACGT", b"TGCA")


@pytest.fixture(scope="module")
def dev():
    from kman_amd import engine

    return engine.default_device()


# ------------------------------------------------------------ kernel vs numpy


@functools.lru_cache(maxsize=None)
def _keys(n: int, W: int = 1) -> np.ndarray:
    """(W, n) planes of sorted distinct rows (row order = plane 0, then 1, ..)."""
    rng = np.random.default_rng(1000 + n + W)
    k0 = (np.cumsum(rng.integers(1, 1000, n, dtype=np.int64)).astype(np.uint64) + np.uint64(1 << 40))
    planes = [k0] + [rng.integers(0, 1 << 63, n, dtype=np.int64).astype(np.uint64) for _ in range(W - 1)]
    out = np.stack(planes) if n else np.zeros((W, 0), np.uint64)
    out.setflags(write=False)
    return out


def _range(cb: int):
    """(lo, hi, kept values, dropped values): u64 counts sit above 2^32, with
    dropped values whose low 32 bits are inside the range."""
    if cb == 4:
        return 2, 5, [2, 3, 5], [1, 6, 9, B32 - 1]
    return B32 + 2, B32 + 5, [B32 + 2, B32 + 3, B32 + 5], [3, B32 + 1, B32 + 6, 2 * B32 + 3]


@functools.lru_cache(maxsize=None)
def _counts(n: int, pattern: str, cb: int) -> np.ndarray:
    rng = np.random.default_rng(7 * n + len(pattern) + cb)
    _, _, keep_v, drop_v = _range(cb)
    i = np.arange(n)
    keep = {
        "all": np.ones(n, bool), "none": np.zeros(n, bool), "alternating": i % 2 == 0, "first_row": i == 0,
        "last_row": i == n - 1, "last_tile": i >= (max(n, 1) - 1) // T * T, "not_first_tile": i >= T,
        "random": rng.random(n) < 0.4,
    }[pattern]
    kv = np.asarray(keep_v, np.uint64)[rng.integers(0, len(keep_v), n)]
    dv = np.asarray(drop_v, np.uint64)[rng.integers(0, len(drop_v), n)]
    out = np.where(keep, kv, dv).astype(np.uint32 if cb == 4 else np.uint64)
    out.setflags(write=False)
    return out


class _Rows:
    """Key planes and counts on the device, PAD sentinel rows after each."""

    def __init__(self, dev, keys, counts, stride=None, fill=0xA5):
        W, n = keys.shape
        self.dev, self.W, self.n = dev, W, n
        self.stride = max(n, 1) if stride is None else stride
        self.cdt = counts.dtype
        self.hk = np.full(W * self.stride + PAD, np.uint64(0xA5A5A5A5A5A5A5A5), np.uint64)
        for j in range(W):
            self.hk[j * self.stride:j * self.stride + n] = keys[j]
        self.hc = np.full(n + PAD, 0xA5A5A5A5, self.cdt)
        self.hc[:n] = counts
        self.k = dev.alloc(self.hk.nbytes)
        self.c = dev.alloc(self.hc.nbytes)
        dev.upload(self.k, self.hk)
        dev.upload(self.c, self.hc)

    def get(self):
        return self.dev.download(self.k, len(self.hk), np.uint64), self.dev.download(self.c, len(self.hc), self.cdt)

    def free(self):
        self.k.free()
        self.c.free()


def _call(dev, src: _Rows, lo, hi, dst, n=None, at=0):
    """kman_filter_counts of src (from row `at`) into dst (_Rows, or None: count only)."""
    out = c_uint64(12345)
    cb = src.cdt.itemsize
    rc = N.lib().kman_filter_counts(
        dev.ctx, c_void_p(src.k.ptr + 8 * at), src.W, src.stride, c_void_p(src.c.ptr + cb * at), cb,
        src.n - at if n is None else n, lo, hi, c_void_p(dst.k.ptr + 8 * at) if dst else None,
        c_void_p(dst.c.ptr + cb * at) if dst else None, byref(out))
    return rc, int(out.value)


def _check(dev, keys, counts, lo, hi, stride=None, mixed=False, at=0):
    """In place, out of place and count only against numpy; the rows past the
    kept ones, the sentinels and (out of place) the inputs are untouched."""
    W, n = keys.shape
    m = n - at
    cnt = counts[at:].astype(np.uint64)
    keep = (cnt >= np.uint64(lo)) & (cnt <= np.uint64(hi))
    want = int(keep.sum())
    if mixed:
        assert 0 < want < m  # (a test cannot pass by filtering nothing, or everything)
    src = _Rows(dev, keys, counts, stride)
    dst = _Rows(dev, np.zeros_like(keys), np.zeros_like(counts), stride)
    try:
        S = src.stride
        rc, got = _call(dev, src, lo, hi, None, at=at)
        assert (rc, got) == (N.KMAN_OK, want)
        k1, c1 = src.get()
        np.testing.assert_array_equal(k1, src.hk)  # count only: nothing written
        np.testing.assert_array_equal(c1, src.hc)
        # out of place
        d0k, d0c = dst.hk.copy(), dst.hc.copy()
        rc, got = _call(dev, src, lo, hi, dst, at=at)
        assert (rc, got) == (N.KMAN_OK, want)
        k1, c1 = src.get()
        np.testing.assert_array_equal(k1, src.hk)
        np.testing.assert_array_equal(c1, src.hc)
        k2, c2 = dst.get()
        for j in range(W):
            np.testing.assert_array_equal(k2[j * S + at:j * S + at + want], keys[j, at:][keep])
            d0k[j * S + at:j * S + at + want] = keys[j, at:][keep]
        np.testing.assert_array_equal(c2[at:at + want], counts[at:][keep])
        d0c[at:at + want] = counts[at:][keep]
        np.testing.assert_array_equal(k2, d0k)  # (nothing else was written)
        np.testing.assert_array_equal(c2, d0c)
        # in place
        rc, got = _call(dev, src, lo, hi, src, at=at)
        assert (rc, got) == (N.KMAN_OK, want)
        k3, c3 = src.get()
        ek, ec = src.hk.copy(), src.hc.copy()
        for j in range(W):
            ek[j * S + at:j * S + at + want] = keys[j, at:][keep]
        ec[at:at + want] = counts[at:][keep]
        np.testing.assert_array_equal(k3, ek)
        np.testing.assert_array_equal(c3, ec)
    finally:
        src.free()
        dst.free()
    return want


@pytest.mark.parametrize("cb", [4, 8])
@pytest.mark.parametrize("n", SIZES)
def test_filter_matches_numpy(dev, n, cb):
    lo, hi, _, _ = _range(cb)
    for pattern in PATTERNS:
        _check(dev, _keys(n), _counts(n, pattern, cb), lo, hi, mixed=pattern in MIXED and n >= T - 1)


@pytest.mark.parametrize("cb", [4, 8])
def test_lo_equals_hi(dev, cb):
    n = 3 * T + 17
    lo, _, keep_v, _ = _range(cb)
    want = _check(dev, _keys(n), _counts(n, "random", cb), keep_v[1], keep_v[1], mixed=True)
    assert want < int((_counts(n, "random", cb).astype(np.uint64) >= np.uint64(lo)).sum())


@pytest.mark.parametrize("cb", [4, 8])
def test_rows_that_are_not_16_byte_aligned(dev, cb):
    """From row 1 of the arrays (keys at 8, counts at 4 or 8 bytes past an
    aligned address): the scalar-load instances of the kernel."""
    n = 3 * T + 18
    lo, hi, _, _ = _range(cb)
    for pattern in ("random", "not_first_tile", "all"):
        _check(dev, _keys(n), _counts(n, pattern, cb), lo, hi, mixed=pattern == "random", at=1)


@pytest.mark.parametrize("cb", [4, 8])
@pytest.mark.parametrize("W", [2, 3])
def test_word_planes_keep_their_stride(dev, W, cb):
    lo, hi, _, _ = _range(cb)
    for n, stride in ((T + 1, T + 9), (3 * T + 17, 3 * T + 17 + 1001), (5, 5)):
        for pattern in ("random", "alternating", "all", "none", "last_tile"):
            _check(dev, _keys(n, W), _counts(n, pattern, cb), lo, hi, stride=stride, mixed=pattern in MIXED and n > T)


def test_empty_and_refused_calls(dev):
    n = T + 1
    keys, counts = _keys(n), _counts(n, "random", 4)
    src = _Rows(dev, keys, counts)
    dst = _Rows(dev, np.zeros_like(keys), np.zeros_like(counts))
    L = N.lib()
    try:
        assert _call(dev, src, 2, 5, dst, n=0) == (N.KMAN_OK, 0)
        assert _call(dev, src, 6, 5, dst) == (N.KMAN_OK, 0)  # lo > hi
        assert _call(dev, src, 6, 5, None) == (N.KMAN_OK, 0)
        np.testing.assert_array_equal(dst.get()[0], dst.hk)
        out = c_uint64(9)
        kp, cp = src.k.ptr, src.c.ptr
        bad = [
            (kp, cp, kp + 8 * 5, dst.c.ptr),       # output keys inside the input keys
            (kp, cp, dst.k.ptr, cp + 4 * 7),       # output counts inside the input counts
            (kp, cp, kp, dst.c.ptr),               # one output equal, one apart
            (kp, cp, dst.k.ptr, None),             # one output NULL
            (kp, cp, None, dst.c.ptr),
            (kp, cp, dst.k.ptr, dst.k.ptr + 8),    # the outputs overlap each other
        ]
        for a, b, c, d in bad:
            rc = L.kman_filter_counts(dev.ctx, c_void_p(a), 1, n, c_void_p(b), 4, n, 2, 5, c_void_p(c), c_void_p(d),
                                      byref(out))
            assert rc == N.KMAN_EINVAL, (a - kp, c, d)
        assert L.kman_filter_counts(dev.ctx, c_void_p(kp), 1, n, c_void_p(cp), 2, n, 2, 5, None, None,
                                    byref(out)) == N.KMAN_EINVAL  # count_bytes
        assert L.kman_filter_counts(dev.ctx, c_void_p(kp), 2, n - 1, c_void_p(cp), 4, n, 2, 5, None, None,
                                    byref(out)) == N.KMAN_EINVAL  # stride < n
        k1, c1 = src.get()
        np.testing.assert_array_equal(k1, src.hk)
        np.testing.assert_array_equal(c1, src.hc)
        # the context is still usable
        want = int(((counts >= 2) & (counts <= 5)).sum())
        assert _call(dev, src, 2, 5, None) == (N.KMAN_OK, want)
    finally:
        src.free()
        dst.free()


# ----------------------------------------------------------------- engine API


def _motif_text() -> bytes:
    """Random 21-mers are all singletons: a repeated motif gives counts > 1."""
    import inputs

    return b">r\n" + (b"ACGTTGCAAC" * 3000) + b"\n>s\n" + inputs.syn_numpy(200_000, 9).split(b"\n", 1)[1]


@functools.lru_cache(maxsize=None)
def _np_rows(k: int, canonical: bool = False):
    import np_oracle

    keys, _ = np_oracle.stream_kmers(np_oracle.parse_fasta(_motif_text()), k, canonical=canonical)
    uk, uc = np_oracle.rle_count(np.sort(keys))
    uk.setflags(write=False)
    uc.setflags(write=False)
    return uk, uc


@pytest.mark.parametrize("canonical", [False, True])
@pytest.mark.parametrize("k", [15, 21, 31])
def test_engine_filter_matches_np_oracle(dev, k, canonical):
    from kman_amd import engine

    uk, uc = _np_rows(k, canonical)
    p = engine.parse(dev, _motif_text())
    try:
        top = int(uc.max())  # (the motif's k-mers: about 3000 each)
        for lo, hi in ((2, None), (2, top), (1, 1), (top, top), (1, None)):
            keep = (uc >= lo) & (uc <= (hi if hi is not None else top))
            assert (lo, hi) == (1, None) or 0 < keep.sum() < len(uc)
            r = engine.join_groups(p, k, False, "count", canonical=canonical)
            try:
                n0 = r.n
                assert engine.filter_counts(dev, r, lo, hi) is r
                if (lo, hi) == (1, None):
                    assert r.n == n0 == len(uk)
                else:
                    assert 0 < r.n < n0  # kept and dropped rows both exist
                gk, gc = engine.download_count(dev, r)
                np.testing.assert_array_equal(gk, uk[keep])
                np.testing.assert_array_equal(gc.astype(np.uint64), uc[keep].astype(np.uint64))
            finally:
                engine.free_result(r)
    finally:
        p.free()


def test_join_groups_canonical_ranged_is_refused(dev):
    from kman_amd import engine

    p = engine.parse(dev, _motif_text())
    try:
        with pytest.raises(NotImplementedError, match="RangedJoin"):
            engine.join_groups(p, 21, False, "count", max_keys=50_000, canonical=True)
        with pytest.raises(ValueError):
            engine.join_groups(p, 21, False, "uniq", canonical=True)
    finally:
        p.free()


# ------------------------------------------------------------------------ CLI


def _cli(*argv):
    from kman_amd.scripts.kmer import main

    main([str(a) for a in argv], standalone_mode=False)


def _in_range(text: bytes, lo: int, hi) -> bytes:
    """The lines of a count output whose count is in [lo, hi]."""
    out = []
    for line in text.splitlines():
        c = int(line.split(b"\t")[1])
        if c >= lo and (hi is None or c <= hi):
            out.append(line + b"\n")
    return b"".join(out)


def _canonical_rows(text: bytes) -> bytes:
    return b"".join(line + b"\n" for line in text.splitlines()
                    if line.split(b"\t")[0] <= line.split(b"\t")[0][::-1].translate(_RC))


# golden `count` cases in which [2, 5] keeps some rows and drops others
# (checked on the reference's outputs when this list was written; asserted below)
GOLDEN_CASES = ["edge__count__k3", "edge__count__k5", "edge__count__k2__r", "edge__count__k5__r",
                "messy1__count__k5", "messy1__count__k5__r", "messy1__count__k5__b37", "messy1_gz__count__k5"]


def _golden(name: str):
    import json

    with open(os.path.join(GOLDEN, "manifest.json")) as fh:
        case = [c for c in json.load(fh)["cases"] if c["name"] == name][0]
    with open(os.path.join(GOLDEN, "ref_outputs", name + ".txt"), "rb") as fh:
        return case, fh.read()


@pytest.mark.parametrize("name", GOLDEN_CASES)
def test_count_range_pinned_to_reference_lines(golden_inputs, tmp_path, name):
    case, ref = _golden(name)
    want = _in_range(ref, 2, 5)
    assert 0 < len(want.splitlines()) < len(ref.splitlines())
    out = tmp_path / "got.txt"
    _cli("count", golden_inputs[case["input"]], out, case["k"], *case["flags"], "-L", 2, "-U", 5)
    assert out.read_bytes() == want


@pytest.mark.parametrize("name", ["messy1__count__k5", "messy1__count__k21", "messy1__count__k31",
                                  "messy1__count__k40", "messy1__count__k5__r"])
def test_identity_range_is_byte_identical(golden_inputs, tmp_path, name):
    case, ref = _golden(name)
    out = tmp_path / "got.txt"
    _cli("count", golden_inputs[case["input"]], out, case["k"], *case["flags"], "-L", 1)
    assert out.read_bytes() == ref
    if case["k"] >= 21:  # every row is a singleton: -L 2 keeps none, -U 1 all
        _cli("count", golden_inputs[case["input"]], out, case["k"], *case["flags"], "-L", 2)
        assert out.read_bytes() == b""
        _cli("count", golden_inputs[case["input"]], out, case["k"], *case["flags"], "--max-count", 1)
        assert out.read_bytes() == ref


@pytest.fixture(scope="module")
def motif(tmp_path_factory, oracle_bin):
    """The repeated-motif input and the oracle's `count` output per (k, -r)."""
    d = tmp_path_factory.mktemp("motif")
    src = d / "motif.fa"
    src.write_bytes(_motif_text())
    cache = {}

    def rows(k: int, rc: bool = False) -> bytes:
        if (k, rc) not in cache:
            out = d / ("want_%d_%d.txt" % (k, rc))
            subprocess.run([oracle_bin, "count", str(src), str(out), str(k)] + (["-r"] if rc else []), check=True)
            cache[k, rc] = out.read_bytes()
        return cache[k, rc]

    return str(src), rows


@pytest.mark.parametrize("k, flags, lo, hi", [
    (21, [], 2, None), (21, [], 2, 5000), (31, [], 2, None), (40, [], 2, None), (40, [], 1, 1), (70, [], 3, 3000),
    (21, ["-r"], 2, 6000), (21, ["-b", 50_000], 2, None),
], ids=lambda v: str(v))
def test_count_range_matches_oracle_on_repeats(motif, tmp_path, k, flags, lo, hi):
    """k = 21, 31: the region path; 40, 70: word planes (W = 2, 3); -b: batches."""
    src, rows = motif
    ref = rows(k, "-r" in flags)
    want = _in_range(ref, lo, hi)
    assert 0 < len(want.splitlines()) < len(ref.splitlines())
    out = tmp_path / "got.txt"
    _cli("count", src, out, k, *flags, "-L", lo, *(["-U", hi] if hi is not None else []))
    assert out.read_bytes() == want


def test_count_range_np_oracle_rows_through_the_command(motif, tmp_path):
    """The same pin from np_oracle's rows (k = 21), formatted by the host writer."""
    from kman_amd import engine

    uk, uc = _np_rows(21)
    keep = (uc >= 2) & (uc <= 5000)
    assert 0 < keep.sum() < len(uc)
    out = tmp_path / "got.txt"
    _cli("count", motif[0], out, 21, "--min-count", 2, "--max-count", 5000)
    assert out.read_bytes() == engine.format_count(uk[keep], uc[keep].astype(np.uint32), 21)


def test_python_m_command(motif, tmp_path):
    src, rows = motif
    out = tmp_path / "got.txt"
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    for v in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "KMAN_DIST"):
        env.pop(v, None)
    subprocess.run([sys.executable, "-m", "kman_amd", "count", src, str(out), "21", "-L", "2", "-U", "5000"],
                   check=True, env=env, cwd=ROOT)
    want = _in_range(rows(21), 2, 5000)
    assert 0 < len(want) < len(rows(21)) and out.read_bytes() == want


def test_filter_with_reloaded_batches(motif, tmp_path):
    """-B reloads go through the gathered join: filtered like the rest."""
    src, rows = motif
    _cli("batch", src, tmp_path / "b", 21, "-b", 60_000)
    out = tmp_path / "got.txt"
    _cli("count", src, out, 21, "-B", tmp_path / "b", "-L", 2)
    want = _in_range(rows(21), 2, None)
    assert 0 < len(want) < len(rows(21)) and out.read_bytes() == want


def test_fastq_quality_mask_and_min_count(tmp_path, oracle_bin):
    import fastq_cases as fq
    from fastq_qual_cases import mask_fastq

    text = fq.short_reads(300_000)
    fasta, _ = mask_fastq(text, 20, 33)
    (tmp_path / "reads.fq").write_bytes(text)
    (tmp_path / "q20.fa").write_bytes(fasta)
    subprocess.run([oracle_bin, "count", str(tmp_path / "q20.fa"), str(tmp_path / "want.txt"), "9"], check=True)
    ref = (tmp_path / "want.txt").read_bytes()
    want = _in_range(ref, 2, None)
    assert 0 < len(want.splitlines()) < len(ref.splitlines())
    _cli("count", tmp_path / "reads.fq", tmp_path / "got.txt", 9, "-q", 20, "-L", 2)
    assert (tmp_path / "got.txt").read_bytes() == want


def _rc_cases():
    import json

    with open(os.path.join(GOLDEN, "manifest.json")) as fh:
        cases = json.load(fh)["cases"]
    return [c for c in cases if c["cmd"] == "count" and c["flags"] == ["-r"] and c["k"] % 2 == 1
            and os.path.isfile(os.path.join(GOLDEN, "ref_outputs", c["name"] + ".txt"))]


@pytest.mark.parametrize("case", _rc_cases(), ids=lambda c: c["name"])
def test_canonical_command_pinned_by_reference_rc_counts(golden_inputs, tmp_path, case):
    """`count --canonical` = the reference's `count -r` rows with seq <= rc(seq) (odd k)."""
    _, ref = _golden(case["name"])
    want = _canonical_rows(ref)
    assert 0 < len(want) < len(ref)
    out = tmp_path / "got.txt"
    _cli("count", golden_inputs[case["input"]], out, case["k"], "--canonical")
    assert out.read_bytes() == want


@pytest.mark.parametrize("name, hi", [("edge__count__k3__r", None), ("edge__count__k5__r", None),
                                      ("messy1__count__k5__r", 5)])
def test_canonical_command_with_min_count(golden_inputs, tmp_path, name, hi):
    case, ref = _golden(name)
    rows = _canonical_rows(ref)
    want = _in_range(rows, 2, hi)
    assert 0 < len(want) < len(rows)
    out = tmp_path / "got.txt"
    _cli("count", golden_inputs[case["input"]], out, case["k"], "--canonical", "-L", 2,
         *(["-U", hi] if hi is not None else []))
    assert out.read_bytes() == want


def test_canonical_on_repeats_matches_oracle(motif, tmp_path):
    src, rows = motif
    want = _in_range(_canonical_rows(rows(21, True)), 2, None)
    assert want
    out = tmp_path / "got.txt"
    _cli("count", src, out, 21, "--canonical", "-L", 2, "-b", 70_000)
    assert out.read_bytes() == want


def test_kjoiner_canonical_needs_one_whole_forward_stream(dev, motif, tmp_path):
    from kman_amd.batcher import FastaBatcher
    from kman_amd.join import KJoiner

    j = KJoiner(KJoiner.MODE.SEQ_COUNT)
    j.canonical = True
    out = tmp_path / "got.txt"
    batches = FastaBatcher(size=100_000, reverse=True, device=dev).do(motif[0], 21).collection
    with pytest.raises(AssertionError, match="without"):
        j.join(batches, str(out))
    batches = FastaBatcher(size=100_000, device=dev).do(motif[0], 21).collection
    with pytest.raises(AssertionError, match="whole"):
        j.join(batches[:-1], str(out))  # (not the whole stream)
    assert not out.exists()
    j.join(batches, str(out))
    assert out.read_bytes() == _canonical_rows(motif[1](21, True))


# ------------------------------------------------------------------ multi-GPU


def _ranks_text() -> bytes:
    """A repeat of A / C only, whose k-mers have keys in the lower part of the
    key space, and random bases (singletons at k = 21): the rank with the
    highest keys holds singletons alone."""
    import inputs

    return b">r\n" + (b"AACACCAAAC" * 250) + b"\n>s\n" + inputs.syn_numpy(60_000, 5).split(b"\n", 1)[1]


@pytest.mark.parametrize("G", [2, 3])
def test_filter_under_simulated_ranks(G, tmp_path):
    from kman_amd import dist, engine, shard

    text, k = _ranks_text(), 21
    one = _in_range(engine.count_text(text, k), 2, None)
    assert one
    devs = [engine.Device(0) for _ in range(G)]
    pipes = []
    try:
        rd = shard.BytesReader(text)
        for r in range(G):
            pipes.append(dist.DistPipeline(devs[r], rd, k, "count", G, r, None))
        grp = dist.SimGroup(pipes)
        grp.step()
        before = [p.results() for p in pipes]
        kept = [int((v >= 2).sum()) for _, v in before]
        assert all(len(v) for _, v in before) and 0 in kept and sum(kept) == len(one.splitlines())
        for p in pipes:
            p.count_range = (2, None)
        got = tmp_path / "got.txt"
        grp.run(lambda p: p.emit_gen(str(got)))
        assert got.read_bytes() == one
        for p, (bk, bv) in zip(pipes, before):  # the pipeline's own rows are as they were
            ak, av = p.results()
            np.testing.assert_array_equal(ak, bk)
            np.testing.assert_array_equal(av, bv)
        # (and the unfiltered text still is the whole output)
        for p in pipes:
            p.count_range = (1, None)
        grp.run(lambda p: p.emit_gen(str(tmp_path / "all.txt")))
        assert (tmp_path / "all.txt").read_bytes() == engine.count_text(text, k)
    finally:
        for p in pipes:
            p.free()
        for d in devs:
            d.close()
