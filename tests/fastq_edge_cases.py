"""FASTQ parse test helper (not a conftest): texts that put every event of the
four-line parse and of the quality mask on a chunk, tile or scan-block edge of
kman_parse_fastq / kman_parse_fastq_q, and an independent statement of the
result.  Pure Python and numpy; never imports the GPU.

``cases()`` maps a name to ``(text, meta)``.  ``meta`` says where the event
sits: ``family``, ``at`` (a byte offset), ``byte`` (``text[at]``; ``"base"`` =
a sequence letter; None = not stated), ``before`` (``text[at - 1]``) and
``kind`` (the line kind, 0 header .. 3 quality, of the line that holds
``text[at]``; ``starts``: ``at`` starts that line).  Family ``qmask`` adds
``T`` (the threshold byte) and ``masked`` (the code indices that must be
masked); family ``errors`` adds ``message`` (None: the text is valid).  Header
and sequence bytes are below 0x80; quality bytes may be 0x21..0xff.

The statement: records and codes are ``expected(text)`` (fastq_to_fasta ->
np_oracle.parse_fasta / codes_of), masked results ``expected(text, T)``
(fastq_qual_cases.mask_fastq), header offsets ``header_offsets(text)``.

The functions under "the model" compute, from that statement alone, the
quantities the parser's geometry depends on (a sequence line's offset in its
64-byte chunk, the codes before it, a tile's code count, ...).  They decide
nothing about the expected result; the CPU test uses them to assert that the
cases reach the geometry they are meant to reach.
"""

from __future__ import annotations

import functools

import numpy as np

import fasta_cases as fa
import fastq_cases as fq
from fastq_qual_cases import mask_fastq

# The internal sizes of kman_amd/csrc/fastq.hip: PB, PTILE and SCAN_T * PTILE.
CHUNK = 64
TILE = 16384
BLOCK = 1024 * TILE

EDGES = [63, 64, 65, TILE - 1, TILE, TILE + 1, TILE + 63, TILE + 64, TILE + 65, 2 * TILE - 1, 2 * TILE]
LF, CR, SP = 0x0A, 0x0D, 0x20
KINDS = ("header", "sequence", "plus", "quality")
NLS = {"lf": b"\n", "crlf": b"\r\n", "cr": b"\r"}
EXOTIC = b"\t\x0b\x0c\x1c\x1d\x1e\x1f"  # stripped only when trailing
LETTERS = b"ACGTacgtN"
T_PLAIN = 0x35  # '5': the threshold byte the plain families are run under

FAMILIES = ("line_start_at", "lone_cr_at", "emit_align", "multi_run", "trailing_ws", "eof_at", "qmask", "errors",
            "scan_block")
LARGE_NAMES = ("big_plus_qual_block", "big_hdr_seq_block", "big_seq_at_block_masked")

MSG_AT = "FASTQ record %d: header line does not start with '@'"
MSG_PLUS = "FASTQ record %d: separator line does not start with '+'"
MSG_LEN = "FASTQ record %d: quality length %d != sequence length %d"


# ------------------------------------------------------------ the statement


def line_table(text: bytes):
    """(bytes as u8, line-start offsets, n_eff): the universal-newline rule of
    fasta_cases.line_starts; n_eff lines remain once the trailing empty ones
    are dropped."""
    b = np.frombuffer(text, dtype=np.uint8)
    st = np.nonzero(fa.line_starts(text))[0]
    nonempty = np.nonzero((b[st] != LF) & (b[st] != CR))[0] if len(st) else st
    return b, st, (int(nonempty[-1]) + 1 if len(nonempty) else 0)


def header_offsets(text: bytes) -> np.ndarray:
    """The offset of every fourth line start, the trailing empty lines dropped."""
    _, st, n_eff = line_table(text)
    return st[0:n_eff:4].astype(np.uint64)


def expected(text: bytes, qbyte: int = 0):
    """(n_records, codes, rec_seq, n_masked) of a valid text; under a threshold
    byte the codes of the masked records.  AssertionError with the parser's
    message for a text that breaks a rule."""
    import np_oracle

    if qbyte:
        fasta, n_masked = mask_fastq(text, qbyte - 33, 33)
    else:
        fasta, n_masked = fq.fastq_to_fasta(text), 0
    recs = np_oracle.parse_fasta(fasta)
    codes, rec_seq = np_oracle.codes_of(recs)
    return len(recs), codes, rec_seq, n_masked


def requal(text: bytes, T: int = T_PLAIN) -> bytes:
    """The text with every quality byte replaced by T - 1 or T, decided by the
    byte's offset alone (about a quarter become T - 1)."""
    b, st, _ = line_table(text)
    b = b.copy()
    li = np.cumsum(fa.line_starts(text)) - 1
    off = np.arange(len(b), dtype=np.uint64)
    isq = ((li & 3) == 3) & (b != LF) & (b != CR)
    low = ((off * np.uint64(2654435761)) >> np.uint64(7)) & np.uint64(3) == 0
    b[isq] = np.where(low[isq], T - 1, T).astype(np.uint8)
    return b.tobytes()


# ---------------------------------------------------------------- the model


def _is_ws(b):
    return (b == SP) | ((b >= 9) & (b <= 13)) | ((b >= 0x1C) & (b <= 0x1F))


def layout(text: bytes):
    """(seq_off, qual_off) of a valid text: the text offset of every kept
    sequence byte (code i comes from text[seq_off[i]]) and of its quality byte
    (same column, two lines on)."""
    b, st, _ = line_table(text)
    n = len(b)
    li = np.cumsum(fa.line_starts(text)) - 1
    off = np.arange(n, dtype=np.int64)
    content = (b != LF) & (b != CR)
    last_nonws = np.maximum.reduceat(np.where(content & ~_is_ws(b), off, -1), st) if n else off
    kept = ((li & 3) == 1) & content & (b != SP) & (off <= last_nonws[li])
    seq_off = np.nonzero(kept)[0]
    g = li[seq_off]
    st2 = np.concatenate([st, [n, n]])  # (a sequence line kept bytes come from has a line two on in a valid text)
    return seq_off, seq_off - st[g] + st2[g + 2]


def codes_before(text: bytes) -> np.ndarray:
    """cb[x] = the number of codes that come from text[:x], for x in 0..len."""
    kept = np.zeros(len(text), dtype=np.int64)
    kept[layout(text)[0]] = 1
    return np.concatenate([[0], np.cumsum(kept)])


def lines_before(text: bytes) -> np.ndarray:
    return np.concatenate([[0], np.cumsum(fa.line_starts(text))])


def tile_bases(text: bytes) -> np.ndarray:
    """The codes before every tile, and (last entry) in the whole text."""
    cb = codes_before(text)
    return np.concatenate([cb[0:len(text):TILE], cb[-1:]])


def chunk_runs(text: bytes):
    """Per 64-byte chunk that holds kept sequence bytes: (chunk, runs, a, cb,
    cnt) -- the number of maximal runs of them, the offset of the first in the
    chunk, the codes before the chunk's first, and how many the chunk holds."""
    n = len(text)
    nch = -(-n // CHUNK)
    kept = np.zeros(nch * CHUNK, dtype=np.int8)
    kept[layout(text)[0]] = 1
    cb = np.concatenate([[0], np.cumsum(kept, dtype=np.int64)])
    m = kept.reshape(nch, CHUNK)
    cnt = m.sum(axis=1)
    runs = (np.diff(np.concatenate([np.zeros((nch, 1), np.int8), m], axis=1), axis=1) == 1).sum(axis=1)
    a = m.argmax(axis=1)
    ch = np.nonzero(cnt)[0]
    return [(int(c), int(runs[c]), int(a[c]), int(cb[c * CHUNK]), int(cnt[c])) for c in ch]


def coverage(text: bytes) -> dict:
    """The geometry a valid text reaches.  c1: (a, codes before mod 4) of the
    single-run chunks; c2: (a & 3, last code's index mod 4) of them; tile_lines
    / chunk_lines: lines-before mod 4 of the tiles / chunks with sequence
    bytes; lk31: (al + lk0) & 31 of the full single-run chunks; multi: chunks
    with more than one run."""
    runs = chunk_runs(text)
    lb = lines_before(text)
    tb = tile_bases(text)
    out = dict(c1=set(), c2=set(), tile_lines=set(), chunk_lines=set(), lk31=set(), multi=set())
    for c, r, a, cb, cnt in runs:
        out["chunk_lines"].add(int(lb[c * CHUNK]) & 3)
        out["tile_lines"].add(int(lb[c * CHUNK // TILE * TILE]) & 3)
        if r == 1:
            out["c1"].add((a, cb & 3))
            out["c2"].add((a & 3, (cb + cnt - 1) & 3))
            if cnt == CHUNK:
                base = int(tb[c * CHUNK // TILE])
                out["lk31"].add(((base & 15) + cb - base) & 31)
        else:
            out["multi"].add(c)
    return out


def shared_vectors(text: bytes):
    """tile_base mod 16 of the tiles that hold a code and whose first (unless
    tile_base mod 16 is 0: then no vector is shared on that side) and last
    16-byte output vectors each hold a code of the neighbour tile too."""
    tb = tile_bases(text)
    kept = np.diff(tb)
    out = set()
    for t in range(0, len(kept) - 1):
        al, end = int(tb[t]) & 15, int(tb[t + 1])
        if kept[t] >= 1 and (al == 0 or (t and kept[t - 1] >= 1)) and end & 15 and kept[t + 1] >= 1 and kept[t] >= 32:
            out.add(al)
    return out


# ---------------------------------------------------------------- builders

_P = [.24, .24, .24, .24, .01, .01, .01, .005, .005]


def _seq(rng, n: int) -> bytes:
    return rng.choice(np.frombuffer(LETTERS, np.uint8), n, p=_P).tobytes() if n else b""


def _qual(rng, n: int, i: int = 0) -> bytes:
    """n quality bytes of '!'..'~'; every third line begins with '@', '+' or '>'."""
    q = bytearray(rng.integers(0x21, 0x7F, n, dtype=np.uint8).tobytes()) if n else bytearray()
    if n and i % 3 == 0:
        q[0] = b"@+>"[(i // 3) % 3]
    return bytes(q)


def _rec(rng, name: bytes, s: int, nl: bytes = b"\n", plus: bytes = b"+", terms=None, i: int = 0, seq=None,
         qual=None) -> bytes:
    t = terms or (nl,) * 4
    seq = _seq(rng, s) if seq is None else seq
    qual = _qual(rng, len(seq), i) if qual is None else qual
    return b"@" + name + t[0] + seq + t[1] + plus + t[2] + qual + t[3]


def _fill(rng, n: int, nl: bytes = b"\n", read_len: int = 100, codes_mod16=None) -> bytes:
    """Exactly n bytes of whole records (2 + name + 2 s + 4 len(nl) bytes
    each); codes_mod16: their base count mod 16."""
    t = len(nl)
    if n == 0:
        return b""
    assert n >= 4 * t + 3, n
    unit = 5 + 2 * read_len + 4 * t
    room = 4 * t + 44  # (the last record keeps 18 bases or more)
    out, left, i, codes = [], n, 0, 0
    while left >= unit + room:
        out.append(_rec(rng, b"f%02d" % (i % 100), read_len, nl, i=i))
        left -= unit
        codes += read_len
        i += 1
    body = left - 4 * t - 2  # name + 2 s
    if codes_mod16 is None:
        nm = 1 if (body - 1) % 2 == 0 else 2
        s = (body - nm) // 2
    else:
        s = (body - 1) // 2
        s -= (s + codes - codes_mod16) % 16
        nm = body - 2 * s
    assert s >= 0 and nm >= 1
    out.append(_rec(rng, b"g" * nm, s, nl, i=i))
    text = b"".join(out)
    assert len(text) == n
    return text


def _tail(rng, nl: bytes = b"\n") -> bytes:
    return b"".join(_rec(rng, b"tail%d" % j, s, nl, i=j) for j, s in enumerate((100, 37, 64)))


def _around(rng, X: int, rec: bytes, off: int, nl: bytes = b"\n", tail: bool = True) -> bytes:
    """Whole records, then `rec` with rec[off] at byte X, then _tail."""
    text = _fill(rng, X - off, nl) + rec
    assert text[X] == rec[off]
    return text + (_tail(rng, nl) if tail else b"")


def _char(c: int) -> str:
    return chr(c)


def _n_records(text: bytes) -> int:
    return len(fq.fastq_lines(text)) // 4


def _with_quals(text: bytes, T: int, masked) -> bytes:
    """Every quality byte T, but T - 1 under the codes listed."""
    b, st, _ = line_table(text)
    b = b.copy()
    li = np.cumsum(fa.line_starts(text)) - 1
    b[((li & 3) == 3) & (b != LF) & (b != CR)] = T
    _, qual_off = layout(text)
    b[qual_off[np.asarray(sorted(masked), dtype=np.int64)]] = T - 1
    return b.tobytes()


def _some(lo: int, hi: int):
    """A fixed quarter of the indices lo..hi-1, lo and hi - 1 among them."""
    return sorted({lo, hi - 1} | {i for i in range(lo, hi) if ((i * 2654435761) >> 5) % 4 == 0})


# ---- C


def _emit_c1(rng, a_values, nl: bytes) -> bytes:
    """Per a: four records whose sequence line starts at offset a of its chunk
    with lengths all 1 mod 4 (or all 3 mod 4), so the codes before them take
    every residue mod 4; then one of an even length.  Headers of 64 bytes or
    more keep two sequence lines out of one chunk."""
    t = len(nl)
    out, p, i = [], 0, 0
    for gi, a in enumerate(a_values):
        ring = [1, 5, 65, 129] if a % 2 == 0 else [3, 63, 127, 3]
        todo = [(a, ring[(gi + j) % 4]) for j in range(4)] + [((a * 7 + 13) % 64, [2, 4, 64, 128][gi % 4])]
        for aa, L in todo:
            nm = 64 + (aa - (p + 1 + t)) % 64
            r = _rec(rng, (b"c%d_" % i).ljust(nm, b"x"), L, nl, i=i)
            assert (p + 1 + nm + t) % 64 == aa
            out.append(r)
            p += len(r)
            i += 1
    return b"".join(out)


C3_K, C3_S = 7, 100


def _emit_c3(rng) -> bytes:
    """16 blocks of exactly one tile of whole records behind a first record of
    C3_S + 4 + C3_K bytes: every tile edge falls C3_K bytes before the end of
    a sequence line.  The blocks' base counts mod 16 (6, then 1 fourteen times,
    then 3) make tile_base mod 16 run 0, 1, .. 15, 2: no tile but the first
    starts, and none ends, on a whole output vector."""
    first = _rec(rng, b"first", 50)
    assert len(first) == C3_S + 4 + C3_K
    out = [first]
    for j in range(16):
        last = _rec(rng, b"z", C3_S, i=j)
        step = 6 if j == 0 else (3 if j == 15 else 1)
        out.append(_fill(rng, TILE - len(last), codes_mod16=(step - C3_S) % 16) + last)
    return b"".join(out)


# ---- E


def _ws_run(c: int, n: int, spaces: bool) -> bytes:
    ab = (b" " + EXOTIC + b" ") if spaces else EXOTIC
    return bytes([c]) + bytes(ab[(3 * j + 1) % len(ab)] for j in range(n - 1))


def _trailing(rng, X: int, c: int, variant: str):
    """A record whose sequence line has its byte X - 1 == c, bases before it;
    -> (text, the sequence line's content)."""
    head = _seq(rng, 20).replace(b"N", b"A")
    if variant == "i":
        seq = head + _ws_run(c, 6, True)
    elif variant == "ii":
        seq = head + _ws_run(c, 150, True)
    elif variant == "iii":
        seq = head + _ws_run(c, 150, True) + b"G"
    elif variant == "v_nl":
        seq = head + bytes([c]) + b" \t \t\t  \t" * 9
    elif variant == "v_base":
        seq = head + bytes([c]) + b" \t \t\t  \t" * 9 + b"C"
    else:
        raise KeyError(variant)
    rec = _rec(rng, b"ws", 0, seq=seq, qual=_qual(rng, len(seq), 1))
    return _around(rng, X - 1, rec, 4 + len(head)), seq


# ---- the small cases


@functools.lru_cache(maxsize=None)
def small_cases() -> dict:
    rng = np.random.default_rng(20261)
    out = {}

    def add(name, text, **meta):
        assert name not in out, name
        meta.setdefault("byte", None)
        meta.setdefault("before", None)
        out[name] = (text, meta)

    # A: each line kind starts at X; the split \r|\n pair at X
    for nlname, nl in NLS.items():
        t = len(nl)
        for X in EDGES:
            s = 20 if X < 200 else 150
            starts = [0, 2 + t, 2 + t + s + t, 3 + s + 3 * t]
            lens = [2, s, 1, s]
            for k in range(4):
                text = _around(rng, X, _rec(rng, b"e", s, nl, i=k), starts[k], nl)
                add("ls_%s_%s_at_%d" % (KINDS[k], nlname, X), text, family="line_start_at", at=X, kind=k, starts=True,
                    byte=["@", "base", "+", None][k], before=nl[-1:].decode())
                if nlname == "crlf":
                    text = _around(rng, X, _rec(rng, b"e", s, nl, i=k), starts[k] + lens[k] + 1, nl)
                    add("split_crlf_%s_at_%d" % (KINDS[k], X), text, family="line_start_at", at=X, kind=k, starts=False,
                        byte="\n", before="\r")

    # B: a lone \r before the edge in a \n file
    for X in (64, TILE, TILE + 64):
        s = 20 if X < 200 else 150
        starts = [0, 3, 4 + s, 6 + s]
        for k in range(4):
            b = bytearray(_around(rng, X, _rec(rng, b"e", s, i=k + 1), starts[k]))
            assert b[X - 1] == LF
            b[X - 1] = CR
            add("lone_cr_%s_at_%d" % (KINDS[k], X), bytes(b), family="lone_cr_at", at=X, kind=k, starts=True,
                byte=["@", "base", "+", None][k], before="\r")

    # C: single-run chunks through the barrel shifter and the tile write-out
    add("emit_c1_lo", _emit_c1(rng, range(0, 32), b"\n"), family="emit_align", at=0, byte="@")
    add("emit_c1_hi", _emit_c1(rng, range(32, 64), b"\r\n"), family="emit_align", at=0, byte="@")
    add("emit_c3", _emit_c3(rng), family="emit_align", at=TILE, byte="base", before="base", kind=1, starts=False,
        many_tiles=True)

    # D: several runs in one chunk
    for X in (64, TILE):
        for ph in range(4):
            tiny = b"".join(_rec(rng, b"abcdefghij"[j % 10:j % 10 + 1], 1 + (j + ph) % 5, i=j) for j in range(44))
            text = _around(rng, X, tiny, 150 + 3 * ph if X > 200 else 45 + 3 * ph)
            add("multi_run_tiny_at_%d_p%d" % (X, ph), text, family="multi_run", at=X,
                multi=[X // CHUNK - 1, X // CHUNK, X // CHUNK + 1] if X > 200 else [1, 2], tiny=True)
        for ph in range(3):
            seq = bytearray(_seq(rng, 330))
            seq[3 + ph::7] = b" " * len(seq[3 + ph::7])
            seq[0:1], seq[-1:] = b"A", b"T"
            rec = _rec(rng, b"sp", 0, seq=bytes(seq), qual=_qual(rng, len(seq), ph))
            text = _around(rng, X, rec, 4 + (170 if X > 200 else 30) + ph)
            add("multi_run_spaces_at_%d_p%d" % (X, ph), text, family="multi_run", at=X, kind=1, starts=False,
                multi=[X // CHUNK - 1, X // CHUNK, X // CHUNK + 1] if X > 200 else [1, 2], tiny=False)

    # E: the whitespace probe (variant iv, the text ending in the run, breaks rule 2: family H)
    for X in (64, TILE):
        for c in EXOTIC:
            for variant in ("i", "ii", "iii", "v_nl", "v_base"):
                text, seq = _trailing(rng, X, c, variant)
                add("trailing_ws_%d_x%02x_%s" % (X, c, variant), text, family="trailing_ws", at=X - 1, kind=1,
                    starts=False, byte=_char(c), before="base", variant=variant, line=seq)

    # F: the text ends on an edge
    for X in (63, 64, 65, TILE - 1, TILE, TILE + 1):
        for end, nl, cut in (("qual", b"\n", 1), ("lf", b"\n", 0), ("cr", b"\r", 0), ("crlf", b"\r\n", 0)):
            text = _fill(rng, X + cut, nl)[:X]
            add("eof_at_%d_%s" % (X, end), text, family="eof_at", at=X - 1, kind=3, starts=None, length=X, end=end,
                byte={"lf": "\n", "cr": "\r", "crlf": "\n"}.get(end), before="\r" if end == "crlf" else None)
    blanks = (b"\n\r\n\n\n\r\n\r\n\n" * (2 * TILE // 10 + 10))[:2 * TILE + 25]
    text = _fill(rng, TILE - 10) + blanks
    add("eof_blank_tiles", text, family="eof_at", at=TILE - 10, byte="\n", before="\n", length=3 * TILE + 15,
        end="blank")
    text = _fill(rng, TILE + 100) + b"@r\n\n+"
    add("eof_cut_record", text, family="eof_at", at=len(text) - 1, kind=2, starts=True, byte="+", before="\n",
        length=TILE + 105, end="cut")

    # G: the quality mask
    T = T_PLAIN

    def add_q(name, text, masked, T=T, **meta):
        masked = sorted(int(i) for i in masked)
        add(name, _with_quals(text, T, masked), family="qmask", T=T, masked=masked, **meta)

    for read_len in range(100, 132):
        base = _fill(rng, 2 * TILE + 500, read_len=read_len)
        tb1 = int(tile_bases(base)[1])
        if 2 <= tb1 & 15 <= 14:
            break
    lo = tb1 - (tb1 & 15)
    for nm, idx in (("first_of_tile", tb1), ("last_of_tile", tb1 - 1), ("shared_lo", lo), ("shared_hi", lo + 15)):
        add_q("qmask_g1_" + nm, base, [idx], at=TILE, g="g1", tile_base=tb1)

    for where in (0, TILE + 200):
        pre = _fill(rng, where) if where else b""
        tb = int(tile_bases(pre + b"@")[-2]) if where else 0  # the codes before the tile the block lies in
        al, cb, p = tb & 15, (sum(len(x) for x in fq.fastq_lines(pre)[1::4]) if where else 0), len(pre)
        recs, masked = [], []
        for s31 in range(32):
            for nm in range(1, 65):
                s1 = p + 2 + nm
                first = cb + (-s1) % 64
                if (al + first - tb) & 31 == s31:
                    break
            L = (-s1) % 64 + 64 + 5 + s31 % 7
            recs.append(_rec(rng, b"q" * nm, L, i=s31))
            masked += [first, first + 63]
            p += len(recs[-1])
            cb += L
        text = pre + b"".join(recs) + _tail(rng)
        assert len(text) <= (where // TILE + 1) * TILE
        add_q("qmask_g2_tile%d" % (where // TILE), text, masked, at=where, g="g2", byte="@")

    for nlname, nl in NLS.items():
        text = _fill(rng, 300, nl) + b"".join(
            _rec(rng, b"p%d" % j, 150 + j // 4, nl, plus=b"+" + b"x" * (j % 4), i=j) for j in range(8))
        add_q("qmask_g3_" + nlname, text, _some(0, int(tile_bases(text)[-1])), at=300, g="g3", byte="@")

    for shape in ("single", "multi"):
        for tiles_on, dist in ((1, TILE), (2, 2 * TILE)):
            seq = bytearray(_seq(rng, 100))
            if shape == "multi":
                seq[5::9] = b" " * len(seq[5::9])
            pre = _fill(rng, 130)
            rec = _rec(rng, b"far", 0, seq=bytes(seq), plus=b"+" + b"far " * (dist // 4) + b"x" * (dist % 4 + 70),
                       qual=_qual(rng, len(seq), 1))
            text = pre + rec + _tail(rng)
            nb = int(tile_bases(pre)[-1])
            add_q("qmask_g4_%s_%d_on" % (shape, tiles_on), text, _some(nb, nb + len(bytes(seq).replace(b" ", b""))),
                  at=130, g="g4", byte="@", shape=shape, tiles_on=tiles_on)
    pre = _fill(rng, 200)
    nb = int(tile_bases(pre)[-1])
    text = pre + _rec(rng, b"long", TILE + 300) + _tail(rng)
    add_q("qmask_g4_long_read", text, _some(nb, nb + TILE + 300), at=200, g="g4", byte="@", shape="single", tiles_on=1)

    for r in range(4):
        pre = _fill(rng, 300)
        nm, L = [(nm, L) for nm in (1, 2) for L in (70, 71) if (305 + nm + 2 * L) % 4 == r][0]
        text = pre + _rec(rng, b"l" * nm, L)[:-1]
        assert len(text) % 4 == r
        nb = int(tile_bases(text)[-1])
        add_q("qmask_g5_mod%d_last_low" % r, text, [nb - L, nb - 1], at=len(text) - 1, g="g5", kind=3, starts=False)
        add_q("qmask_g5_mod%d_last_high" % r, text, [nb - L, nb - 2], at=len(text) - 1, g="g5", kind=3, starts=False)

    text = _fill(rng, 3 * TILE + 300)
    tb = tile_bases(text)
    add_q("qmask_g6_full_tile", text, range(int(tb[1]), int(tb[2])), at=TILE, g="g6")

    text = _around(rng, TILE, _rec(rng, b"e", 150), 3)
    tb1 = int(tile_bases(text)[1])
    add_q("qmask_g7_record_start", text, [tb1], at=TILE, g="g7", kind=1, starts=True, byte="base", before="\n",
          code12=tb1)

    text = _fill(rng, 600) + b"".join(_rec(rng, b"w%d" % j, 150 + j, i=j) for j in range(5))
    for T8, ring in ((0x9D, (0x21, 0x7F, 0x80, 0x9C, 0x9D, 0xFF, 0x9C)), (0x80, (0x7F, 0x80, 0x21, 0xFF, 0x81)),
                     (0x81, (0x80, 0x81, 0x7F, 0xFF, 0x21, 0x82))):
        b = np.frombuffer(_with_quals(text, T8, []), np.uint8).copy()
        _, qual_off = layout(text)
        vals = np.array([ring[i % len(ring)] for i in range(len(qual_off))], dtype=np.uint8)
        b[qual_off] = vals
        add("qmask_g8_T%02x" % T8, b.tobytes(), family="qmask", T=T8, masked=np.nonzero(vals < T8)[0].tolist(),
            at=600, g="g8", byte="@")

    # H: errors (message None: valid)
    def bad(name, text, message, **meta):
        add("err_" + name, text, family="errors", message=message, **meta)

    def straddle(rule):
        pre = _fill(rng, TILE - 120)
        r = _n_records(pre) + 1
        seq, qual = _seq(rng, 200), _qual(rng, 200, 1)
        rec = {1: b"xh\n" + seq + b"\n+\n" + qual + b"\n", 2: b"@h\n" + seq + b"\n-\n" + qual + b"\n",
               3: b"@h\n" + seq + b"\n+\n" + qual[:-3] + b"\n"}[rule]
        msg = {1: MSG_AT % r, 2: MSG_PLUS % r, 3: MSG_LEN % (r, 197, 200)}[rule]
        return pre + rec + _tail(rng), msg

    for rule in (1, 2, 3):
        text, msg = straddle(rule)
        bad("rule%d_straddles_tile" % rule, text, msg, at=TILE - 120)
    pre = _fill(rng, 5000)
    r = _n_records(pre) + 1
    text = pre + b"@a\nACGTA\n+\nIIII\n" + _fill(rng, TILE + 300 - len(pre) - 16) + b"no at\nAC\n+\nII\n" + _tail(rng)
    bad("two_offenders_lower_record", text, MSG_LEN % (r, 4, 5), at=5000)
    text = _fill(rng, 700) + b"rules 1 and 3\nACGT\n+\nII\n" + _tail(rng)
    bad("rules_1_and_3", text, MSG_AT % (_n_records(_fill(rng, 700)) + 1), at=700)
    text = _fill(rng, TILE - 90) + b"@m\r\n" + _seq(rng, 150) + b"\r\n+\n" + _qual(rng, 150) + b"\n" + _tail(rng)
    bad("valid_seq_crlf_qual_lf", text, None, at=TILE - 90)
    text = _fill(rng, TILE - 90) + b"@m\n" + _seq(rng, 150) + b"\n+\r\n" + _qual(rng, 150) + b"\r\n" + _tail(rng)
    bad("valid_seq_lf_qual_crlf", text, None, at=TILE - 90)
    pre = _fill(rng, TILE - 60)
    r = _n_records(pre) + 1
    bad("len_one_short_at_end", pre + b"@z\n" + _seq(rng, 90) + b"\n+\n" + b"I" * 89, MSG_LEN % (r, 89, 90),
        at=TILE - 60)
    bad("len_one_long_at_end", pre + b"@z\n" + _seq(rng, 90) + b"\n+\n" + b"I" * 91, MSG_LEN % (r, 91, 90),
        at=TILE - 60)
    for X in (64, TILE):
        for c in EXOTIC:
            # E iv: a final record cut short in its sequence line, which ends the text in whitespace
            pre = _fill(rng, X - 1 - 24)
            text = pre + b"@ws\n" + _seq(rng, 20) + _ws_run(c, 150, True)
            assert text[X - 1] == c
            bad("trailing_ws_%d_x%02x_iv" % (X, c), text, MSG_PLUS % (_n_records(pre) + 1), at=X - 1, kind=1,
                starts=False, byte=_char(c), before="base")
    return out


# ---------------------------------------------------------------- the large


@functools.lru_cache(maxsize=None)
def _pool():
    """997 records of one size as rows of bytes: 120-byte names, 60 bases."""
    rng = np.random.default_rng(77)
    K, NM, S = 997, 120, 60
    m = np.empty((K, 1 + NM + 1 + S + 3 + S + 1), dtype=np.uint8)
    m[:, 0] = ord("@")
    m[:, 1:1 + NM] = rng.choice(np.frombuffer(b"abcdefghijklmnopqrstuvwxyz0123456789_:/", np.uint8), (K, NM))
    m[:, 1 + NM] = LF
    m[:, 2 + NM:2 + NM + S] = rng.choice(np.frombuffer(LETTERS, np.uint8), (K, S), p=_P)
    m[:, 2 + NM + S:5 + NM + S] = np.frombuffer(b"\n+\n", np.uint8)
    m[:, 5 + NM + S:5 + NM + 2 * S] = rng.integers(0x21, 0x7F, (K, S), dtype=np.uint8)
    m[:, -1] = LF
    return m


def _big_fill(n: int) -> bytes:
    """Exactly n bytes of whole records, built with numpy."""
    m = _pool()
    K, U = m.shape
    units = (n - 600) // U
    reps = -(-units // K)
    body = np.tile(m, (reps, 1))[:units].tobytes()
    return body + _fill(np.random.default_rng(n % 1000), n - len(body))


@functools.lru_cache(maxsize=1)
def large_case(name: str):
    """One text of just over 1024 tiles (16 MiB): built when asked for."""
    rng = np.random.default_rng(LARGE_NAMES.index(name))
    tail = _fill(rng, 2 * TILE + 777)
    if name == "big_plus_qual_block":
        # '+' starts at BLOCK - 1, the quality line at BLOCK + 1: three lines of the record lie before the block
        rec = b"@b\nA\n+\n@\n"
        text = _big_fill(BLOCK - 1 - 5) + rec + tail
        return text, dict(family="scan_block", at=BLOCK - 1, byte="+", before="\n", kind=2, starts=True,
                          also=(BLOCK + 1, 3))
    if name == "big_hdr_seq_block":
        # '@' starts at BLOCK - 1 (an empty name), the sequence line at BLOCK + 1
        rec = b"@\n" + _seq(rng, 150) + b"\n+\n" + _qual(rng, 150) + b"\n"
        text = _big_fill(BLOCK - 1) + rec + tail
        return text, dict(family="scan_block", at=BLOCK - 1, byte="@", before="\n", kind=0, starts=True,
                          also=(BLOCK + 1, 1))
    if name == "big_seq_at_block_masked":
        rec = _rec(rng, b"blk", 150)
        text = _big_fill(BLOCK - 5) + rec + tail
        first = int(np.searchsorted(layout(text)[0], BLOCK))
        masked = sorted({first, first + 1, first + 149, first - 1, 0} | set(_some(first - 4000, first + 4000)))
        return _with_quals(text, T_PLAIN, masked), dict(family="scan_block", at=BLOCK, byte="base", before="\n", kind=1,
                                                         starts=True, T=T_PLAIN, masked=masked, code12=first)
    raise KeyError(name)


def cases() -> dict:
    """Every case, the large ones included (about 50 MB of text)."""
    out = dict(small_cases())
    for name in LARGE_NAMES:
        out[name] = large_case(name)
    return out
