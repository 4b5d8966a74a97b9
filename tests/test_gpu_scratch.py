"""No device buffer outlives the call that made it: every DeviceBuffer
allocated during a lookup function is freed when the function returns or
raises, except the buffers it returns and the caller's own index."""

from __future__ import annotations

import contextlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

K = 5
SEQ40 = b"ACGTTGCAAGGCTTAACCGGATATCGCGTACGTTGCAAGG"
# records of 5, 40 and 0 bases
READS = b"@r1\nACGTA\n+\nIIIII\n@r2 x\n" + SEQ40 + b"\n+\n" + b"I" * 40 + b"\n@r3\n\n+\n\n"
# an interleaved input: two pairs (5 + 40 bases, 0 + 12 bases)
PAIRS = (b"@a/1\nACGTA\n+\nIIIII\n@a/2\n" + SEQ40 + b"\n+\n" + b"I" * 40 + b"\n@b/1\n\n+\n\n@b/2\n" + SEQ40[:12]
         + b"\n+\n" + b"I" * 12 + b"\n")
OTHER = b">ref2\nTTGCAAGGCTTAACCAAAAAAC\n"


@pytest.fixture(scope="module")
def dev():
    from kman_amd import engine

    return engine.default_device()


@contextlib.contextmanager
def recorded(dev, monkeypatch):
    """Every DeviceBuffer that dev.alloc makes inside the block, in a list."""
    made, alloc = [], dev.alloc

    def recording(nbytes):
        made.append(alloc(nbytes))
        return made[-1]

    with monkeypatch.context() as m:
        m.setattr(dev, "alloc", recording, raising=False)
        yield made


def _live(made, returned=()):
    return [b for b in made if b.ptr is not None and not any(b is r for r in returned)]


def _table(dev, text):
    from kman_amd import engine

    p = engine.parse(dev, text)
    try:
        return engine.join_groups(p, K, False, "count")
    finally:
        p.free()


@pytest.fixture()
def world(dev):
    """(reads, the pair view's two parses, table of the reads, coloured table
    of two references), parsed afresh for every test: correct() patches codes."""
    from kman_amd import engine

    p = engine.parse(dev, READS, keep_text=True)
    pm = engine.parse(dev, PAIRS)
    pv = engine.pairs_of(pm)
    table = _table(dev, READS)
    ctable = engine.color_table(dev, [_table(dev, READS), _table(dev, OTHER)])
    assert p.n_records == 3 and p.rec_seq.tolist() == [0, 5, 45] and p.n_bases == 45 and table.n > 0
    yield p, pm, pv, table, ctable
    for x in (p, pv, pm):
        x.free()
    engine.free_result(table)
    engine.free_result(ctable)


@pytest.mark.parametrize("own_index", [False, True], ids=["index_none", "caller_index"])
def test_every_lookup_frees_what_it_allocates(dev, world, monkeypatch, own_index):
    from kman_amd import engine

    p, pm, pv, table, ctable = world
    index = engine.table_index(dev, table) if own_index else None
    cindex = engine.table_index(dev, ctable) if own_index else None
    calls = [
        ("screen", lambda: engine.screen(p, table, index=index)),
        ("screen_median", lambda: engine.screen_median(p, table, index=index)),
        ("screen_solid", lambda: engine.screen_solid(p, table, False, 2, median=True, index=index)),
        ("classify", lambda: engine.classify(p, ctable, 2, index=cindex, planes=True)),
        ("screen_pairs", lambda: engine.screen_pairs(pm, pv, table, median=True, min_count=2, index=index)),
        ("filter_counts", lambda: engine.filter_counts(dev, table, 1, 1 << 40)),
        ("correct", lambda: engine.correct(p, table, False, 2, index=index)),
    ]
    try:
        for name, call in calls:
            with recorded(dev, monkeypatch) as made:
                call()
            assert made or name == "filter_counts", name
            assert _live(made) == [], name
        with recorded(dev, monkeypatch) as made:
            d_wc = engine.window_counts(p, table, index=index)
        try:
            assert d_wc.ptr is not None and any(b is d_wc for b in made)
            assert _live(made, (d_wc,)) == []
            for name, call in (("record_runs", lambda: engine.record_runs(p, d_wc, 2)),
                               ("record_quantile", lambda: engine.record_quantile(p, d_wc))):
                with recorded(dev, monkeypatch) as made:
                    call()
                assert made and _live(made) == [], name
        finally:
            d_wc.free()
        with recorded(dev, monkeypatch) as made:
            idx = engine.table_index(dev, table)
        assert _live(made, (idx,)) == [] and idx.ptr is not None
        idx.free()
        if own_index:
            assert index.ptr is not None and cindex.ptr is not None  # (the caller's are not the callee's to free)
    finally:
        for b in (index, cindex):
            if b is not None:
                b.free()


def test_a_refused_argument_after_the_first_allocation_leaves_nothing(dev, world, monkeypatch):
    """Ordinary Python errors raised by argument checks that run after device
    buffers were made: the index and the window counts of screen_median are
    there when record_quantile refuses 2 / 1, and cut_records has uploaded its
    offsets when the span arrays turn out to be of the wrong length."""
    from kman_amd import engine

    p, pm, pv, table, ctable = world
    with recorded(dev, monkeypatch) as made:
        with pytest.raises(AssertionError, match="quantile 2 / 1"):
            engine.screen_median(p, table, num=2, den=1)
    assert len(made) >= 2 and _live(made) == []
    with recorded(dev, monkeypatch) as made:
        with pytest.raises(AssertionError, match="span arrays of"):
            engine.cut_records(p, None, span=(np.zeros(1, np.uint64), np.zeros(1, np.uint64)), trim=True)
    assert len(made) >= 1 and _live(made) == []
    assert p.text.ptr is not None and p.codes.ptr is not None
