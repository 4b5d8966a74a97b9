"""The FASTQ edge cases (tests/fastq_edge_cases.py) without a GPU: every
case's premise holds of its text, every valid case is valid under the restated
rule and every error case raises exactly its message, the listed masked codes
are what mask_fastq masks, and the coverage conditions hold -- the geometry of
fastq.hip the cases are meant to reach (C1-C3, the bit-map shifts, the line
counts mod 4 before tiles and chunks), computed from the statement alone.  The
GPU test is only as good as these conditions."""

from __future__ import annotations

import numpy as np
import pytest

import fasta_cases as fa
import fastq_cases as fq
import fastq_edge_cases as fe
from fastq_qual_cases import mask_fastq

TILE, CHUNK, BLOCK = fe.TILE, fe.CHUNK, fe.BLOCK


@pytest.fixture(scope="module")
def small():
    return fe.small_cases()


@pytest.fixture(scope="module")
def cover(small):
    """name -> coverage(text) of the valid cases, computed once."""
    return {name: fe.coverage(text) for name, (text, meta) in small.items() if meta.get("message") is None}


def _is(text, at, what):
    if what is None:
        return True
    if what == "base":
        return text[at] in fe.LETTERS
    return text[at:at + 1] == what.encode("latin-1")


def _check_meta(name, text, meta):
    at = meta["at"]
    assert 0 <= at < len(text), name
    assert _is(text, at, meta["byte"]), name
    assert at == 0 or _is(text, at - 1, meta["before"]), name
    ls = fa.line_starts(text)
    if "kind" in meta:
        assert (int(np.cumsum(ls)[at]) - 1) & 3 == meta["kind"], name
        if meta.get("starts") is not None:
            assert bool(ls[at]) == meta["starts"], name
    if "length" in meta:
        assert len(text) == meta["length"], name
    # header and sequence bytes are below 0x80
    b = np.frombuffer(text, np.uint8)
    assert not np.any((b >= 0x80) & (((np.cumsum(ls) - 1) & 3) < 2)), name


def test_premises_small(small):
    fams = {}
    for name, (text, meta) in small.items():
        _check_meta(name, text, meta)
        fams.setdefault(meta["family"], []).append(name)
        # three tiles; the C3 sweep needs a tile per residue mod 16 and one after them
        assert len(text) <= (17 * TILE if meta.get("many_tiles") else 3 * TILE + 1024), name
    assert sum(len(small[n][0]) for n in fams["emit_align"]) < 400 << 10
    assert set(fams) | {"scan_block"} == set(fe.FAMILIES)
    for fam in fams:
        assert fams[fam], fam
    at = {f: {(small[n][1]["at"], small[n][1].get("kind")) for n in fams[f]} for f in fams}
    for x in fe.EDGES:
        for k in range(4):
            assert (x, k) in at["line_start_at"], (x, k)
            assert "split_crlf_%s_at_%d" % (fe.KINDS[k], x) in small
            for nl in fe.NLS:
                assert small["ls_%s_%s_at_%d" % (fe.KINDS[k], nl, x)][1]["starts"]
    for x in (64, TILE, TILE + 64):
        for k in range(4):
            assert (x, k) in at["lone_cr_at"], (x, k)


def test_valid_cases_are_valid_and_errors_raise_their_message(small):
    n_err = 0
    for name, (text, meta) in small.items():
        if meta.get("message") is None:
            fq.fastq_to_fasta(text)
            fq.fastq_to_fasta(fe.requal(text))
        else:
            n_err += 1
            with pytest.raises(AssertionError) as e:
                fq.fastq_to_fasta(text)
            assert str(e.value) == meta["message"], name
            with pytest.raises(AssertionError) as e:
                mask_fastq(text, 20)
            assert str(e.value) == meta["message"], name
    assert n_err == 7 + 2 * len(fe.EXOTIC)


def test_header_offsets(small):
    """Every fourth line of fastq_lines starts where header_offsets says."""
    for name, (text, meta) in small.items():
        hdr = fe.header_offsets(text).astype(np.int64)
        lines = fq.fastq_lines(text)
        assert len(hdr) == len(lines) // 4, name
        for o, ln in zip(hdr.tolist(), lines[0::4]):
            assert text[o:o + len(ln)] == ln and (o == 0 or text[o - 1] in b"\r\n"), name
        assert np.all(np.diff(hdr) > 0), name
    assert fe.header_offsets(b"@r\n\n+").tolist() == [0]
    assert fe.header_offsets(b"@r\nA\n+\nI\n\n\r\n\n").tolist() == [0]
    assert fe.header_offsets(b"@r\rA\r+\rI\r@s\r\nC\r\n+\r\nI").tolist() == [0, 9]
    assert fe.header_offsets(b"\n\r\n").tolist() == []


def test_requal_keeps_everything_but_quality_bytes(small):
    for name in ("ls_quality_crlf_at_64", "trailing_ws_64_x09_iii", "eof_at_16385_qual", "multi_run_tiny_at_16384_p1"):
        text = small[name][0]
        new = fe.requal(text)
        la, lb = fq.fastq_lines(text), fq.fastq_lines(new)
        assert len(new) == len(text) and len(la) == len(lb)
        for i, (x, y) in enumerate(zip(la, lb)):
            if i % 4 == 3:
                assert len(x) == len(y) and set(y) <= {fe.T_PLAIN - 1, fe.T_PLAIN}
            else:
                assert x == y
        q = b"".join(lb[3::4])
        assert len(q) < 8 or 0 < q.count(bytes([fe.T_PLAIN - 1])) < len(q)


def test_layout_model_is_the_mask_rule(small):
    """code i comes from text[seq_off[i]]: the model's kept bytes are the
    statement's cleaned sequences, so its quantities are the statement's."""
    for name, (text, meta) in small.items():
        if meta.get("message") is not None:
            continue
        seq_off, qual_off = fe.layout(text)
        _, codes, _, _ = fe.expected(text)
        b = np.frombuffer(text, np.uint8)
        import np_oracle

        np.testing.assert_array_equal(np_oracle._CODE[b[seq_off]], codes & 7, err_msg=name)
        assert np.all(qual_off < len(text)), name


# ------------------------------------------------------------- coverage: C


def test_c1_every_chunk_offset_and_codes_before_mod_4(small, cover):
    got = cover["emit_c1_lo"]["c1"] | cover["emit_c1_hi"]["c1"]
    assert {(a, r) for a in range(64) for r in range(4)} <= got
    for name in ("emit_c1_lo", "emit_c1_hi"):
        assert not cover[name]["multi"], name  # single-run chunks only
    lens = {len(ln) for n in ("emit_c1_lo", "emit_c1_hi") for ln in fq.fastq_lines(small[n][0])[1::4]}
    assert lens == {1, 2, 3, 4, 5, 63, 64, 65, 127, 128, 129}


def test_c2_every_start_and_end_byte_lane(cover):
    got = cover["emit_c1_lo"]["c2"] | cover["emit_c1_hi"]["c2"]
    assert {(a, e) for a in range(4) for e in range(4)} == got


def test_c3_every_output_alignment_with_both_end_vectors_shared(small):
    assert fe.shared_vectors(small["emit_c3"][0]) == set(range(16))


# --------------------------------------------------------- coverage: D, E, F


def test_multi_run_chunks(small, cover):
    for name, (text, meta) in small.items():
        if meta["family"] != "multi_run":
            continue
        runs = {c: r for c, r, _, _, _ in fe.chunk_runs(text)}
        for c in meta["multi"]:
            assert runs[c] >= (4 if meta["tiny"] else 2), (name, c)
        edge = meta["at"] // CHUNK
        assert edge - 1 in meta["multi"] or meta["at"] == 64
        assert edge in meta["multi"]
        if meta["tiny"]:
            hdr = fe.header_offsets(text).astype(np.int64) // CHUNK
            assert max(np.bincount(hdr)) >= 4, name
        else:
            assert b" " in fq.fastq_lines(text)[1::4][fe._n_records(text[:meta["at"]]) - 1]
    # a line of each shape straddles the tile edge
    straddled = {(m["tiny"], int(np.cumsum(fa.line_starts(t))[TILE] - 1) & 3, bool(fa.line_starts(t)[TILE]))
                 for t, m in small.values() if m["family"] == "multi_run" and m["at"] == TILE}
    assert any(tiny and not starts for tiny, _, starts in straddled)
    assert (False, 1, False) in straddled


def test_trailing_ws_premises(small):
    seen = set()
    for name, (text, meta) in small.items():
        if meta["family"] != "trailing_ws":
            continue
        X, line, v = meta["at"] + 1, meta["line"], meta["variant"]
        lines = fq.fastq_lines(text)
        r = lines.index(line)
        assert r % 4 == 1 and len(lines[r + 2]) == len(line), name
        start = X - 1 - 20
        assert text[start:start + len(line)] == line and text[start + len(line)] == 0x0A, name
        run = line[20:].rstrip(b"ACGTacgtN") if v in ("iii", "v_base") else line[20:]
        assert not run.strip(b" " + fe.EXOTIC) and line[:20].isalpha(), name
        assert (len(run) > 64) == (v != "i"), name
        if v.startswith("v"):
            assert set(run[1:]) == {0x20, 0x09}, name
        kept = fe.expected(text)[1]
        n_line = 20 + (len(run) - run.count(b" ") + 1 if v in ("iii", "v_base") else 0)
        seq_off = fe.layout(text)[0]
        assert int(((seq_off >= start) & (seq_off < start + len(line))).sum()) == n_line, name
        assert len(kept) == len(seq_off)
        seen.add((X, text[X - 1], v))
    assert seen == {(X, c, v) for X in (64, TILE) for c in fe.EXOTIC for v in ("i", "ii", "iii", "v_nl", "v_base")}
    # variant iv, the text ending in the run, is an error of rule 2
    for X in (64, TILE):
        for c in fe.EXOTIC:
            text, meta = small["err_trailing_ws_%d_x%02x_iv" % (X, c)]
            assert meta["message"].endswith("separator line does not start with '+'")
            assert text[X - 1] == c and not text[X - 1:].strip(b" " + fe.EXOTIC) and len(text) > X + 64


def test_eof_premises(small):
    seen = set()
    for name, (text, meta) in small.items():
        if meta["family"] != "eof_at":
            continue
        end = meta["end"]
        seen.add((meta["length"], end))
        if end == "qual":
            assert text[-1] >= 0x21 and len(fq.fastq_lines(text)[-1]) > 0
        elif end in ("lf", "cr"):
            assert text[-1:] == fe.NLS[end] and text[-2] >= 0x21
        elif end == "crlf":
            assert text[-2:] == b"\r\n"
    assert {(X, e) for X in (63, 64, 65, TILE - 1, TILE, TILE + 1) for e in ("qual", "lf", "cr", "crlf")} <= seen
    text, meta = small["eof_blank_tiles"]
    assert not text[meta["at"]:].strip(b"\r\n") and b"\r\n" in text[meta["at"]:] and b"\n\n" in text[meta["at"]:]
    assert meta["at"] < TILE and len(text) - TILE > 2 * TILE
    text, meta = small["eof_cut_record"]
    assert text.endswith(b"\n@r\n\n+") and len(text) > TILE


# ------------------------------------------------------------- coverage: G


def test_qmask_listed_codes_are_what_mask_fastq_masks(small):
    for name, (text, meta) in small.items():
        if meta["family"] != "qmask":
            continue
        T = meta["T"]
        _, plain, _, _ = fe.expected(text)
        _, codes, _, n_masked = fe.expected(text, T)
        assert n_masked == len(meta["masked"]) == len(set(meta["masked"])) > 0, name
        want = plain.copy()
        want[meta["masked"]] = 4 | (plain[meta["masked"]] & 8)
        np.testing.assert_array_equal(codes, want, err_msg=name)
        if meta["g"] != "g8":
            assert set(b"".join(fq.fastq_lines(text)[3::4])) <= {T - 1, T}, name
        if "code12" in meta:
            assert codes[meta["code12"]] == 12 and meta["code12"] in meta["masked"], name


def test_qmask_geometry(small, cover):
    g = {}
    for name, (text, meta) in small.items():
        if meta["family"] == "qmask":
            g.setdefault(meta["g"], []).append(name)
    assert set(g) == {"g%d" % i for i in range(1, 9)}
    # G1: the tile's first and last code and both sides of the shared vector
    tb1 = small["qmask_g1_first_of_tile"][1]["tile_base"]
    assert 1 <= tb1 & 15 <= 15
    got = {n: small["qmask_g1_" + n][1]["masked"] for n in ("first_of_tile", "last_of_tile", "shared_lo", "shared_hi")}
    assert got == {"first_of_tile": [tb1], "last_of_tile": [tb1 - 1], "shared_lo": [tb1 & ~15],
                   "shared_hi": [(tb1 & ~15) + 15]}
    assert int(fe.tile_bases(small["qmask_g1_shared_lo"][0])[1]) == tb1 and got["shared_lo"][0] < tb1 - 1
    assert got["shared_hi"][0] > tb1
    # G2: a full single-run chunk at every bit-map shift, its first and last code masked alone
    for name in g["g2"]:
        text, meta = small[name]
        tb = fe.tile_bases(text)
        masked = set(meta["masked"])
        shifts = set()
        for c, r, a, cb, cnt in fe.chunk_runs(text):
            if r == 1 and cnt == CHUNK and cb in masked and cb + 63 in masked \
                    and not masked & set(range(cb + 1, cb + 63)):
                base = int(tb[c * CHUNK // TILE])
                shifts.add(((base & 15) + cb - base) & 31)
        assert shifts == set(range(32)), name
    assert int(fe.tile_bases(small["qmask_g2_tile1"][0])[1]) & 15
    # G3: the quality line's distance mod 4, per newline kind
    for name in g["g3"]:
        seq_off, qual_off = fe.layout(small[name][0])
        assert set(((qual_off - seq_off) & 3).tolist()) == {0, 1, 2, 3}, name
        assert not cover[name]["multi"]
    # G4: the quality byte lies one tile, and two tiles, after its base
    seen = set()
    for name in g["g4"]:
        text, meta = small[name]
        seq_off, qual_off = fe.layout(text)
        m = np.asarray(meta["masked"])
        d = set((qual_off[m] // TILE - seq_off[m] // TILE).tolist())
        assert d == {meta["tiles_on"]} or name == "qmask_g4_long_read", name
        multi = bool(set((seq_off[m] // CHUNK).tolist()) & cover[name]["multi"])
        assert multi == (meta["shape"] == "multi"), name
        seen.add((meta["shape"], meta["tiles_on"]))
    assert seen == {(s, t) for s in ("single", "multi") for t in (1, 2)}
    # G5: the quality line ends the text, at every length mod 4, its last byte low and not
    assert {(len(small[n][0]) % 4, small[n][0][-1] < small[n][1]["T"]) for n in g["g5"]} == \
        {(r, low) for r in range(4) for low in (False, True)}
    for n in g["g5"]:
        assert small[n][0][-1] not in b"\r\n" and small[n][1]["kind"] == 3
    # G6: a tile with every code masked between two with none
    text, meta = small["qmask_g6_full_tile"]
    tb = fe.tile_bases(text)
    assert meta["masked"] == list(range(int(tb[1]), int(tb[2]))) and tb[1] > 0 and tb[3] > tb[2] > tb[1]
    # G7: a record's first base, the first code of a tile
    text, meta = small["qmask_g7_record_start"]
    assert meta["masked"] == [int(fe.tile_bases(text)[1])] and int(fe.layout(text)[0][meta["masked"][0]]) == TILE
    # G8: a threshold above 0x80, at 0x80 and at 0x81, quality bytes on both sides of 0x80
    assert {small[n][1]["T"] for n in g["g8"]} == {0x9D, 0x80, 0x81}
    for n in g["g8"]:
        q = set(b"".join(fq.fastq_lines(small[n][0])[3::4]))
        T = small[n][1]["T"]
        assert {T - 1, T} <= q and min(q) < 0x80 < max(q)


# -------------------------------------------------------- global coverage


def test_lines_before_tiles_and_chunks_take_every_residue(small, cover):
    tiles, chunks = set(), set()
    per_family = {}
    for name, cv in cover.items():
        fam = small[name][1]["family"]
        if fam in ("errors", "scan_block"):
            continue
        tiles |= cv["tile_lines"]
        chunks |= cv["chunk_lines"]
        per_family.setdefault(fam, set()).update(cv["tile_lines"])
    assert tiles == {0, 1, 2, 3} and chunks == {0, 1, 2, 3}
    assert per_family["line_start_at"] == {0, 1, 2, 3}


# ------------------------------------------------------------------ errors


def test_error_premises(small):
    msgs = {n[4:]: m["message"] for n, (t, m) in small.items() if m["family"] == "errors"}
    for rule, tail in ((1, "'@'"), (2, "'+'"), (3, "length 197 != sequence length 200")):
        name = "err_rule%d_straddles_tile" % rule
        text, meta = small[name]
        assert msgs[name[4:]].endswith(tail)
        hdr = fe.header_offsets(text).astype(np.int64)
        r = int(msgs[name[4:]].split()[2].rstrip(":")) - 1
        assert hdr[r] < TILE < hdr[r + 1], name  # the record's lines lie on both sides of the edge
    text, meta = small["err_two_offenders_lower_record"]
    assert "quality length 4 != sequence length 5" in meta["message"] and text.index(b"\nno at\n") > TILE > meta["at"]
    assert msgs["valid_seq_crlf_qual_lf"] is None and msgs["valid_seq_lf_qual_crlf"] is None
    assert b"\r\n+\n" in small["err_valid_seq_crlf_qual_lf"][0] and b"\n+\r\n" in small["err_valid_seq_lf_qual_crlf"][0]
    for name, lens in (("len_one_short_at_end", "89 != sequence length 90"), ("len_one_long_at_end", "91 != sequence")):
        assert lens in msgs[name] and small["err_" + name][0].endswith(b"I")


# ------------------------------------------------------------------- large


@pytest.mark.parametrize("name", fe.LARGE_NAMES)
def test_large_case_premises(name):
    text, meta = fe.large_case(name)
    _check_meta(name, text, meta)
    assert meta["family"] == "scan_block" and BLOCK + 2 * TILE < len(text) < BLOCK + 3 * TILE
    ls = fa.line_starts(text)
    lines = np.cumsum(ls)
    assert int(lines[BLOCK - 1]) & 3 != 0  # the lines started before the block edge
    assert BLOCK - 1 <= meta["at"] <= BLOCK + 1 and ls[meta["at"]]
    if "also" in meta:
        at, kind = meta["also"]
        assert BLOCK - 1 <= at <= BLOCK + 1 and ls[at] and (int(lines[at]) - 1) & 3 == kind
    fq.fastq_to_fasta(text)
    hdr = fe.header_offsets(text)
    assert len(hdr) == len(fq.fastq_lines(text)) // 4 > 60_000
    if "masked" in meta:
        seq_off, qual_off = fe.layout(text)
        first = meta["code12"]
        assert int(seq_off[first]) == BLOCK and first in meta["masked"] and first - 1 in meta["masked"]
        b = np.frombuffer(text, np.uint8)
        low = np.nonzero(b[qual_off] < meta["T"])[0]
        assert low.tolist() == meta["masked"]


def test_large_cases_cover_every_line_kind():
    # (metas only: the texts are built once, by the parametrised test)
    kinds = set()
    for name in fe.LARGE_NAMES:
        meta = fe.large_case(name)[1]
        kinds.add(meta["kind"])
        if "also" in meta:
            kinds.add(meta["also"][1])
    assert kinds == {0, 1, 2, 3}
