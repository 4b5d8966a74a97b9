"""`kmer unitigs --gfa` without a GPU: the two plain-Python statements of the
edges between unitigs (tests/gfa_cases.py) held equal on every named case, the
properties include/kman.h states for them, the two host writers against the
statement's text, and the engine's and the command's refusals."""

from __future__ import annotations

import os
import re
from ctypes import byref, c_size_t, c_void_p

import numpy as np
import pytest
from click.testing import CliRunner

import gfa_cases as gc
import unitig_cases as uc

CASES = uc.cases()

# (U, E) as the issue that asked for the links lists them
COUNTS = {"all_3mers": (32, 256), "all_5mers": (512, 4096), "y_fork": (3, 4), "fork_and_merge": (5, 8),
          "poly_a_alone": (1, 2), "poly_a_with_neighbours": (3, 8), "hairpin_k5": (2, 4), "cycle_2": (1, 2),
          "cycle_3": (1, 2), "cycle_500": (1, 2), "cycle_with_tail": (2, 4), "two_cycles_and_paths": (5, 4),
          "acgt_k3": (1, 1)}
COUNTS.update({"path_%d" % n: (1, 0) for n in uc.PATH_NODES})


def _tables(name):
    records, k, min_count = CASES[name]
    yield uc.table_of(records, k, min_count), k
    yield uc.table_of(uc.both_strands(records), k, 2 * min_count - 1), k


@pytest.mark.parametrize("name", sorted(CASES))
def test_both_formulations_agree_and_the_properties_hold(name):
    for table, k in _tables(name):
        units = uc.unitigs(table)
        texts = [s for s, _, _ in units]
        edges = gc.edges_text(texts, k)
        assert edges == gc.edges_rows(table)  # the text and the row formulation: the same list
        have = set(edges)
        assert len(have) == len(edges)  # no edge twice
        for u, o, v, p in edges:
            assert (v, 1 - p, u, 1 - o) in have  # the mirror
            assert gc.oriented(texts[u], o)[-(k - 1):] == gc.oriented(texts[v], p)[:k - 1]  # the overlap
        per_end = np.bincount([2 * u + o for u, o, _, _ in edges], minlength=2 * len(units) + 1)
        assert per_end.max() <= 4 and len(edges) <= 8 * len(units)
        eoff, words = gc.csr(edges, len(units))
        assert len(eoff) == 2 * len(units) + 1 and int(eoff[-1]) == len(edges) == len(words)
        assert gc.uncsr(eoff, words) == edges
        parsed = gc.parse_gfa(gc.gfa_text(units, edges, k))
        assert parsed[0] == [(s, kc) for s, _, kc in units] and parsed[1] == edges
        assert parsed[2] == ({k - 1} if edges else set())
        if name in COUNTS:
            assert (len(units), len(edges)) == COUNTS[name]


def test_the_counts_table_and_the_self_mirror():
    assert set(COUNTS) <= set(CASES)
    records, k, _ = CASES["acgt_k3"]
    units, edges = gc.table_edges(uc.table_of(records, k), k)
    assert edges == [(0, 0, 0, 1)]  # ACG + T = CGT, the first k-mer of revcomp(ACG): its own mirror
    records, k, _ = CASES["all_5mers"]
    units, edges = gc.table_edges(uc.table_of(records, k), k)
    assert np.all(np.diff(gc.csr(edges, len(units))[0]) == 4)  # every end full


def test_tile_edge_cases_have_the_ends_they_name():
    from kman_amd import _native as N

    for name, (records, k, min_count) in gc.tile_cases(N.KMAN_EDGE_TILE).items():
        units, edges = gc.table_edges(uc.table_of(records, k, min_count), k)
        assert 2 * len(units) == int(name.split("_")[1])
        assert 0 < len(edges) < len(units)  # about one component in eight has edges


def _arrays(units):
    off = np.cumsum([0] + [len(s) for s, _, _ in units]).astype(np.uint64)
    seqs = np.frombuffer("".join(s for s, _, _ in units).encode(), dtype=np.uint8).copy()
    return seqs, off, np.asarray([c for _, _, c in units], dtype=np.uint64)


def _call(fn, args, want: bytes):
    """The sizing call, one byte short, then the exact capacity."""
    from kman_amd import _native as N

    used = c_size_t(0)
    rc = fn(*args, None, 0, byref(used), 2)
    if not want:  # (out == NULL is KMAN_ECAP under the kman_format_* contract, whatever the size)
        assert rc == N.KMAN_ECAP and used.value == 0
        one = (N.ctypes.c_char * 1)(b"\xa5")
        assert fn(*args, one, 0, byref(used), 2) == N.KMAN_OK and used.value == 0 and bytes(one) == b"\xa5"
        return
    assert rc == N.KMAN_ECAP and used.value == len(want)
    buf = (N.ctypes.c_char * len(want))()
    used = c_size_t(0)
    assert fn(*args, buf, len(want) - 1, byref(used), 3) == N.KMAN_ECAP and used.value == len(want)
    assert fn(*args, buf, len(want), byref(used), 3) == N.KMAN_OK and used.value == len(want)
    assert bytes(buf) == want


def test_host_writers_agree_with_the_statement():
    from kman_amd import _native as N

    L = N.lib()
    for name in ("two_cycles_and_paths", "all_5mers", "fork_and_merge", "acgt_k3", "path_5000", "empty"):
        records, k, min_count = CASES[name]
        units, edges = gc.table_edges(uc.table_of(records, k, min_count), k)
        U = len(units)
        seqs, off, kc = _arrays(units)
        eoff, words = gc.csr(edges, U)
        p = lambda a: a.ctypes.data_as(c_void_p)  # noqa: E731
        _call(L.kman_format_gfa_segments, (p(seqs), p(off), p(kc), U, 0), gc.segments_text(units))
        _call(L.kman_format_gfa_links, (p(eoff), p(words), U, 0, k), gc.links_text(edges, k))
        # slices: unitigs [a, b) with first_id = a, eoff at the slice's first end, edge at its first edge
        for a, b in ((0, 0), (U, U), (U // 2, U), (1, max(1, U - 1)), (U // 3, U // 3 + 1)):
            if not 0 <= a <= b <= U:
                continue
            _call(L.kman_format_gfa_segments, (p(seqs), c_void_p(off.ctypes.data + 8 * a),
                                               c_void_p(kc.ctypes.data + 8 * a), b - a, a),
                  gc.segments_text(units[a:b], a))
            _call(L.kman_format_gfa_links, (c_void_p(eoff.ctypes.data + 16 * a),
                                            c_void_p(words.ctypes.data + 4 * int(eoff[2 * a])), b - a, a, k),
                  gc.links_text([e for e in edges if a <= e[0] < b], k))
    # numbers of every width, and the writers' own refusals
    big = [("ACGTA", 1, (1 << 64) - 1), ("CC", 1, 0)]
    seqs, off, kc = _arrays(big)
    _call(L.kman_format_gfa_segments, (p(seqs), p(off), p(kc), 2, 99),
          b"S\t99\tACGTA\tLN:i:5\tKC:i:18446744073709551615\nS\t100\tCC\tLN:i:2\tKC:i:0\n")
    eoff = np.asarray([7, 8, 8, 9, 10], dtype=np.uint64)
    words = np.asarray([(1234567 << 1) | 1, 0, 3], dtype=np.uint32)
    _call(L.kman_format_gfa_links, (p(eoff), p(words), 2, 999, 31),
          b"L\t999\t+\t1234567\t-\t30M\nL\t1000\t+\t0\t+\t30M\nL\t1000\t-\t1\t-\t30M\n")
    used = c_size_t(0)
    assert L.kman_format_gfa_segments(None, None, None, 1, 0, None, 0, byref(used), 1) == N.KMAN_EINVAL
    assert L.kman_format_gfa_links(None, None, 1, 0, 21, None, 0, byref(used), 1) == N.KMAN_EINVAL
    assert L.kman_format_gfa_links(p(eoff), None, 2, 0, 21, None, 0, byref(used), 1) == N.KMAN_EINVAL
    for bad_k in (20, 1, 33):
        assert L.kman_format_gfa_links(p(eoff), p(words), 2, 0, bad_k, None, 0, byref(used), 1) == N.KMAN_EINVAL
    down = np.asarray([3, 2, 2, 2, 2], dtype=np.uint64)
    assert L.kman_format_gfa_links(p(down), p(words), 2, 0, 21, None, 0, byref(used), 1) == N.KMAN_EINVAL
    down = np.asarray([5, 2, 7], dtype=np.uint64)
    assert L.kman_format_gfa_segments(p(seqs), p(down), p(kc), 2, 0, None, 0, byref(used), 1) == N.KMAN_EINVAL


def _result(units, k, edges=None):
    from kman_amd import engine

    seqs, off, kc = _arrays(units)
    r = engine.UnitigResult(seqs, off, np.asarray([m for _, m, _ in units], dtype=np.uint32), kc, k)
    if edges is not None:
        r.eoff, r.edges = gc.csr(edges, len(units))
    return r


def test_emit_gfa(monkeypatch, tmp_path):
    from kman_amd import engine

    assert engine.UnitigResult(*_arrays([]), np.zeros(0, np.uint64), 21).eoff is None  # the new fields default to None
    for name in ("two_cycles_and_paths", "all_5mers", "y_fork", "path_17", "empty"):
        records, k, min_count = CASES[name]
        units, edges = gc.table_edges(uc.table_of(records, k, min_count), k)
        want = gc.gfa_text(units, edges, k)
        assert engine.emit_gfa(_result(units, k, edges)) == want
        with open(tmp_path / "out.gfa", "wb") as fh:
            assert engine.emit_gfa(_result(units, k, edges), fh) is None
        assert (tmp_path / "out.gfa").read_bytes() == want
        with pytest.raises(AssertionError, match="links"):
            engine.emit_gfa(_result(units, k))  # a result without links
        assert engine.emit_unitigs(_result(units, k, edges)) == uc.text(units)  # the FASTA writer does not mind them
    assert gc.gfa_text([], [], 21) == b"H\tVN:Z:1.0\n"  # an empty table: the header line alone
    # slices of a few unitigs and a few edges each
    records, k, _ = CASES["all_5mers"]
    units, edges = gc.table_edges(uc.table_of(records, k), k)
    monkeypatch.setattr(engine.unitig, "_UNITIG_SLICE", 37)
    monkeypatch.setattr(engine.unitig, "_GFA_LINK_SLICE", 19)
    assert engine.emit_gfa(_result(units, k, edges)) == gc.gfa_text(units, edges, k)
    r = _result(units, k, edges)
    r.edges = r.edges[:-1]
    with pytest.raises(AssertionError):
        engine.emit_gfa(r)  # fewer edges than the offsets name
    r = _result(units, k, edges)
    r.edges[5] = (len(units) << 1) | 1
    with pytest.raises(AssertionError):
        engine.emit_gfa(r)  # an edge to a unitig that is not there


def test_header_signatures_and_documents():
    from kman_amd import _native as N

    root = os.path.dirname(N.HERE)
    with open(os.path.join(root, "include", "kman.h")) as fh:
        text = fh.read()
    m = re.search(r"#define\s+KMAN_EDGE_TILE\s+(\d+)\s", text)
    assert m and int(m.group(1)) == N.KMAN_EDGE_TILE
    for name, nargs in (("kman_unitig_edges", 15), ("kman_format_gfa_segments", 9), ("kman_format_gfa_links", 9)):
        assert name in N.header_symbols() and len(N.SIGNATURES[name][1]) == nargs, name
        decl = re.search(r"\bint %s\(([^;]*)\);" % name, text)
        assert decl and len(decl.group(1).split(",")) == nargs, name
        assert hasattr(N.lib(), name)
    section = text[text.index("unitigs of a count table"):text.index("#define KMAN_GRAPH_R")]
    assert section.index("Edges between unitigs") < section.index("kman_unitig_edges:")  # the definition first
    section = re.sub(r"\s*\n \*\s*", " ", section)
    for phrase in ("END e = 2 u + o", "is the first k-mer of v's text in orientation p", "ordered by b, A C G T",
                   "Exactly one of the two holds", "(v, !p, u, !o)", "E <= 8 U", "d_eoff[2 U] = E", "(v << 1) | p",
                   "KMAN_ECAP with both numbers set and nothing written", "d_eoff[0] = 0", "KMAN_EDGE_TILE",
                   "two calls give equal bytes", "never a wild address", "56 U bytes", '"unitig_edges"',
                   "Synchronises", "S\\tID\\tSEQ\\tLN:i:BASES\\tKC:i:SUM", "L\\tU\\t+|-\\tV\\t+|-\\t(k-1)M"):
        assert phrase in section, phrase
    with open(os.path.join(N.HERE, "csrc", "unitig.hip")) as fh:
        src = fh.read()
    assert '"unitig_edges"' in src and "table_rows<4>" in src and "layout_kernel<false>" in src
    for doc in ("README.md", "DESIGN.md"):
        with open(os.path.join(root, doc)) as fh:
            body = fh.read()
        assert "--gfa" in body and "kman_unitig_edges" in body and "GFA links between unitigs" not in body


def test_help_and_refusals(tmp_path, monkeypatch):
    from kman_amd import engine
    from kman_amd.scripts.kmer import main

    text = CliRunner().invoke(main, ["unitigs", "--help"]).output
    for word in ("--gfa", "GFA 1.0", "kman_unitig_edges", "colours", "K > 31", "header line alone"):
        assert word in text, word
    assert "GFA links between unitigs" not in text

    def no_device(*a, **kw):
        raise RuntimeError("device work before the options were checked")

    monkeypatch.setattr(engine, "default_device", no_device)
    fa = tmp_path / "a.fa"
    fa.write_bytes(b">s\nTTGCAACGTACGGATTACA\n")
    for argv, msg in (([str(fa), str(tmp_path / "o.gfa.gz"), "21", "--gfa"], "ends in .gz"),
                      ([str(fa), str(tmp_path / "o.gfa"), "20", "--gfa"], "odd K"),
                      ([str(fa), str(fa), "21", "--gfa"], "same file")):
        r = CliRunner().invoke(main, ["unitigs"] + argv)
        assert isinstance(r.exception, AssertionError) and msg in str(r.exception), (r.exception, r.output)
    assert sorted(p.name for p in tmp_path.iterdir()) == ["a.fa"]
    r = CliRunner().invoke(main, ["unitigs", str(fa), str(tmp_path / "o.gfa"), "5", "--gfa"])
    assert isinstance(r.exception, RuntimeError)  # an accepted command reaches the device
