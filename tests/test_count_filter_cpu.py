"""`kmer count` --min-count / --max-count / --canonical without a GPU: the
options exist on `count` alone, every refused combination raises before any
device work or output file, the multi-GPU route of --canonical, and the
KJoiner setters."""

from __future__ import annotations

import pytest
from click.testing import CliRunner


@pytest.fixture()
def fasta(tmp_path):
    p = tmp_path / "in.fa"
    p.write_bytes(b">r\nACGTACGTTGCAACGT\n")
    return p


def test_help_lists_the_options_on_count_only():
    from kman_amd.scripts.kmer import main

    run = CliRunner()
    text = run.invoke(main, ["count", "--help"]).output
    for opt in ("--min-count", "-L,", "--max-count", "-U,", "--canonical"):
        assert opt in text, opt
    for cmd in ("uniq", "batch"):
        text = run.invoke(main, [cmd, "--help"]).output
        for opt in ("--min-count", "--max-count", "--canonical", "-L,", "-U,"):
            assert opt not in text, (cmd, opt)
    text = run.invoke(main, ["hist", "--help"]).output
    assert "--min-count" not in text and "--canonical" not in text
    assert "--max-count" in text and ">=N" in text and "-U" not in text  # (hist's own option keeps its meaning)


REFUSED = {
    "min_above_max": (["-L", "6", "-U", "5"], "greater than"),
    "min_above_max_long": (["--min-count", "3", "--max-count", "2"], "greater than"),
    "min_count_vec": (["-L", "2", "-m", "VEC_COUNT"], "SEQ_COUNT"),
    "max_count_vec_masked": (["-U", "9", "-m", "VEC_COUNT_MASKED"], "SEQ_COUNT"),
    "canonical_vec": (["--canonical", "-m", "VEC_COUNT"], "SEQ_COUNT"),
    "canonical_reverse": (["--canonical", "-r"], "already folded"),
    "canonical_previous_batches": (["--canonical", "-B", "{dir}"], "-B"),
}


@pytest.mark.parametrize("case", sorted(REFUSED))
def test_refused_before_any_device_work_or_output(case, fasta, tmp_path, monkeypatch):
    from kman_amd import _native, engine
    from kman_amd.scripts.kmer import main

    def no_device(*a, **kw):
        raise RuntimeError("device work before the options were checked")

    monkeypatch.setattr(engine, "default_device", no_device)
    monkeypatch.setattr(engine, "Device", no_device)
    monkeypatch.setattr(_native, "lib", no_device)
    flags, msg = REFUSED[case]
    (tmp_path / "batches").mkdir()
    flags = [f.format(dir=tmp_path / "batches") for f in flags]
    out = tmp_path / "out.txt"
    r = CliRunner().invoke(main, ["count", str(fasta), str(out), "3"] + flags)
    assert isinstance(r.exception, AssertionError), (r.exception, r.output)
    assert msg in str(r.exception)
    assert not out.exists() and not (tmp_path / "out").exists()


@pytest.mark.parametrize("flags", [["-L", "0"], ["-U", "0"], ["-L", "x"], ["--max-count", "-3"]])
def test_option_values_below_one_are_usage_errors(flags, fasta, tmp_path):
    from kman_amd.scripts.kmer import main

    out = tmp_path / "out.txt"
    r = CliRunner().invoke(main, ["count", str(fasta), str(out), "3"] + flags)
    assert r.exit_code == 2 and not out.exists()


def test_multi_gpu_canonical_is_solo_rank(tmp_path, monkeypatch):
    from kman_amd.scripts.kmer import _multi_gpu

    fap = tmp_path / "in.fa"
    fap.write_bytes(b">r\nACGT\n")
    for v in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "KMAN_DIST"):
        monkeypatch.delenv(v, raising=False)
    assert _multi_gpu(21, None, "SEQ_COUNT", str(fap), "auto", canonical=True) is False  # no launch
    monkeypatch.setenv("WORLD_SIZE", "4")
    for rank, solo in ((0, False), (2, None)):
        monkeypatch.setenv("RANK", str(rank))
        monkeypatch.setenv("LOCAL_RANK", str(rank))
        assert _multi_gpu(21, None, "SEQ_COUNT", str(fap), "auto", canonical=True) is solo
        assert _multi_gpu(21, None, "SEQ_COUNT", canonical=True) is solo
        # without it: the route from before
        assert _multi_gpu(21, None, "SEQ_COUNT", str(fap), "auto", canonical=False) is True
        assert _multi_gpu(21, None, "SEQ_COUNT", str(fap), "auto") is True
    with pytest.raises(TypeError):  # a trailing keyword: the positional arguments did not move
        _multi_gpu(21, None, "SEQ_COUNT", str(fap), "auto", True)


def test_kjoiner_setters_validate():
    from kman_amd.join import KJoiner, KJoinerThreading

    for cls in (KJoiner, KJoinerThreading):
        j = cls(KJoiner.MODE.SEQ_COUNT)
        assert (j.min_count, j.max_count, j.canonical) == (1, None, False)
        j.min_count, j.max_count, j.canonical = 2, 5, True
        assert (j.min_count, j.max_count, j.canonical) == (2, 5, True)
        j.max_count = None
        assert j.max_count is None
        for bad in (0, -1, 2.0, "2", None, True):
            with pytest.raises(AssertionError):
                j.min_count = bad
        for bad in (0, -1, 5.0, "5", False):
            with pytest.raises(AssertionError):
                j.max_count = bad
        for bad in (0, 1, "yes", None):
            with pytest.raises(AssertionError):
                j.canonical = bad
        assert (j.min_count, j.max_count, j.canonical) == (2, None, True)


@pytest.mark.parametrize("mode", ["UNIQUE", "VEC_COUNT", "VEC_COUNT_MASKED"])
@pytest.mark.parametrize("opt", ["min_count", "max_count", "canonical"])
def test_kjoiner_refuses_the_options_outside_seq_count(mode, opt, tmp_path):
    from kman_amd.join import KJoiner

    j = KJoiner(KJoiner.MODE[mode])
    setattr(j, opt, {"min_count": 2, "max_count": 7, "canonical": True}[opt])
    out = tmp_path / "out.txt"
    with pytest.raises(AssertionError, match="SEQ_COUNT"):
        j.join([], str(out))  # (raised before the batches are looked at)
    assert not out.exists() and not (tmp_path / "out").exists()


def test_kjoiner_refuses_min_above_max(tmp_path):
    from kman_amd.join import KJoiner

    j = KJoiner(KJoiner.MODE.SEQ_COUNT)
    j.min_count, j.max_count = 6, 5
    with pytest.raises(AssertionError, match="greater than"):
        j.join([], str(tmp_path / "out.txt"))
    assert not (tmp_path / "out.txt").exists()


def test_count_range_check():
    from kman_amd import engine

    assert engine.check_count_range() == (1, None)
    assert engine.check_count_range(2, 2) == (2, 2)
    for lo, hi in ((0, None), (1, 0), (3, 2), (True, None), (1.5, None), (1, 2.5)):
        with pytest.raises(AssertionError):
            engine.check_count_range(lo, hi)


def test_join_groups_refuses_canonical_uniq():
    from kman_amd import engine

    with pytest.raises(ValueError, match="canonical"):
        engine.join_groups(None, 21, False, "uniq", canonical=True)


def test_tile_constant_matches_the_header():
    import os
    import re

    from kman_amd import _native as N

    with open(os.path.join(os.path.dirname(N.HERE), "include", "kman.h")) as fh:
        m = re.search(r"#define\s+KMAN_FILTER_TILE\s+(\d+)", fh.read())
    assert m and int(m.group(1)) == N.KMAN_FILTER_TILE
    assert "kman_filter_counts" in N.SIGNATURES and hasattr(N.lib(), "kman_filter_counts")
