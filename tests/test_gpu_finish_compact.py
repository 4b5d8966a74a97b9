"""The plain uniq finish (rg_finish, KMAN_RG_CHECK=0: what the CLI and bench.py
run) lets its last sort pass rank and scatter only the items the early count
marked as singletons, so the pass leaves the region's rows compacted in key
order, and stores each row's key and pos from one LDS read.  The checked
kernel (KMAN_RG_CHECK=1, the GPU session's default) still sorts every item
and compares the marks with the sorted keys; these tests pin the plain one.

Bar: rows, keys and pos, bit-exact against np_oracle (as test_gpu_region.py),
and for the mixed input byte-identical to the checked kernel's rows."""

from __future__ import annotations

from ctypes import byref, c_uint64

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    from kman_amd import engine

    return engine.default_device()


@pytest.fixture(autouse=True)
def plain_finish(monkeypatch):
    """(the kernel reads the variable at every launch)"""
    monkeypatch.setenv("KMAN_RG_CHECK", "0")


def _bases(n, seed):
    rng = np.random.Generator(np.random.PCG64(seed))
    return np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=n, dtype=np.uint8)].tobytes()


def _oracle(text, k, rc):
    import np_oracle

    keys, pos = np_oracle.stream_kmers(np_oracle.parse_fasta(text), k, rc=rc)
    sk, sp = np_oracle.stable_sort(keys, pos)
    return np_oracle.rle_uniq(sk, sp)


def _groups(dev, text, k, rc):
    from kman_amd import engine

    p = engine.parse(dev, text)
    try:
        r = engine.groups(p, k, rc, "uniq")
        assert r is not None, "input inside the region path fell back"
        try:
            return engine.download_uniq(dev, r)
        finally:
            r.keys.free()
            r.pos.free()
    finally:
        p.free()


def _plan(text, k, rc):
    """kman_groups' plan restated (region_groups.hip make_plan, rg_finish's
    pass count of 8-byte items): region bits, key rest bits, finish passes.
    The compacting pass needs the early count, which needs >= 2 passes."""
    import np_oracle
    from kman_amd import _native as N

    n_bases = sum(len(s) for _, s in np_oracle.parse_fasta(text))
    wb = c_uint64(0)
    flags = (N.KMAN_RC if rc else 0) | N.KMAN_WANT_POS
    assert N.lib().kman_groups_plan(n_bases, k, flags, N.KMAN_FINISH_UNIQ, byref(wb)) == N.KMAN_OK
    W = n_bases * (2 if rc else 1)
    b2 = 1
    while b2 < 9 and (W >> (8 + b2)) > 6144:
        b2 += 1
    rest = 2 * k - 8 - b2
    passes = 1 if rest <= 11 else 1 + (rest - 11 + 7) // 8
    return 8 + b2, rest, passes


def _check(dev, text, k, rc):
    _, _, passes = _plan(text, k, rc)
    assert passes >= 2, "this plan's finish has no early count: the case would take the run-length path"
    got = _groups(dev, text, k, rc)
    want = _oracle(text, k, rc)
    np.testing.assert_array_equal(got[0], want[0])
    np.testing.assert_array_equal(got[1].astype(np.uint64), want[1])
    return got, want


@pytest.mark.parametrize("rc", [False, True])
def test_all_singletons(dev, rc):
    """Random sequence, k = 21: every item is marked, the compacting pass
    moves all of them."""
    text = b">a\n" + _bases(150_000, 41) + b"\n"
    _, want = _check(dev, text, 21, rc)
    assert len(want[0]) >= 0.99 * 150_000 * (2 if rc else 1)


def test_full_regions(dev):
    """Regions of ~5.9 K items (3 M bases into 512 regions): the marked items
    of all eight waves, ranked across the per-wave counters."""
    import inputs

    text = inputs.syn_numpy(3_000_000, 43, record_len=1 << 20)
    _check(dev, text, 21, False)


def test_no_rows(dev):
    """A record that holds the same 60 000 bases twice: all but the k-mers
    over the junction occur twice, most regions have no row at all (an empty
    compacting pass, a look-back over zero-row regions)."""
    body = _bases(60_000, 42)
    text = b">twice\n" + body + body + b"\n"
    bits, rest, _ = _plan(text, 21, False)
    _, want = _check(dev, text, 21, False)
    assert len(want[0]) < 100
    assert len(np.unique(want[0] >> np.uint64(rest))) < (1 << bits) // 4


def _mixed(copies):
    rng = np.random.default_rng(copies)
    seg = "".join(rng.choice(list("ACGT"), 300))
    return b">r\n" + _bases(100_000, 3) + b"\n>s\n" + (seg * copies).encode() + b"\n"


@pytest.mark.parametrize("copies", [3, 100])
def test_mixed(dev, copies):
    """The shapes of test_groups_repeats: a 300-base unit repeated beside
    random sequence, duplicates next to singletons in the sorted regions."""
    _, want = _check(dev, _mixed(copies), 21, False)
    assert 99_000 < len(want[0]) < 100_000 + 300


def test_plain_equals_checked(dev, monkeypatch):
    """The rows of the plain kernel are the checked kernel's, byte for byte."""
    text = _mixed(100)
    plain = _groups(dev, text, 21, False)
    monkeypatch.setenv("KMAN_RG_CHECK", "1")
    checked = _groups(dev, text, 21, False)
    assert plain[0].tobytes() == checked[0].tobytes()
    assert plain[1].tobytes() == checked[1].tobytes()


@pytest.mark.parametrize("k,rc", [(13, False), (13, True), (11, False)])
def test_long_runs_of_equal_low_bits(dev, k, rc):
    """A small key space (4^13, 4^11 over 300 000 windows): runs of three and
    more equal low bits (9 of them at k = 13, 5 at k = 11 with its two passes
    and 13 rest bits) reach the LDS scan of the early count, among regions
    where most items are still rows.  (k = 9 has 9 rest bits, one pass and
    no early count: not this path.)"""
    text = b">a\n" + _bases(300_000, 44) + b"\n"
    _check(dev, text, k, rc)


def test_region_rows_at_line_edges(dev):
    """The merged store loop shifts a region's rows by its first row's offset
    in a 64-row line: regions whose row count is a multiple of 64 and one
    more and one less (seeded input; the counts are asserted from the
    oracle's rows), after predecessors of every offset."""
    text = b">a\n" + _bases(150_000, 45) + b"\n"
    bits, rest, _ = _plan(text, 21, False)
    _, want = _check(dev, text, 21, False)
    rows = np.bincount((want[0] >> np.uint64(rest)).astype(np.int64), minlength=1 << bits)
    assert len(rows) == 1 << bits
    for edge in (0, 1, 63):
        assert ((rows % 64 == edge) & (rows > 0)).any(), edge
    firsts = np.concatenate([[0], np.cumsum(rows)[:-1]]) % 64
    assert len(np.unique(firsts)) == 64


def test_round_path_plain():
    """The round path's uniq finish (dist, two simulated ranks): its items
    carry the source rank at tag_shift below the mark bit, and the pos rows
    carry it in bits 56-63."""
    from test_gpu_dist_region import _close, _run, _texts
    from test_gpu_dist_region import _oracle as dist_oracle

    text = _texts()["synth"]
    outs, pipes, _ = _run(text, 21, "uniq", 2)
    try:
        assert all(p.path == "region" for p in pipes)
        tags = np.concatenate([p.results()[1] for p in pipes]) >> np.uint64(56)
        assert set(np.unique(tags).tolist()) == {0, 1}
        wk, wv = dist_oracle(text, 21, "uniq")
        for keys, vals in outs:
            np.testing.assert_array_equal(keys, wk)
            np.testing.assert_array_equal(vals, wv)
    finally:
        _close(pipes)
