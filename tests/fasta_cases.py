"""FASTA parse test helper (not a conftest): texts that put every event of the
parse on a chunk, tile or scan-block edge of kman_parse_fasta, and a second,
independent statement of the reference's rule (kmermaid/parsers.py:86-128,
read in text mode).  Pure Python and numpy; never imports the GPU.

``cases()`` maps a name to ``(text, meta)``.  ``meta`` says where the event
sits: ``family``, ``at`` (a byte offset), ``byte`` (``text[at]``; ``"base"`` =
a sequence letter; None = not stated), ``before`` (``text[at - 1]``) and,
where the case is about the fast path, ``fast_tiles``: the tiles that must be
plain sequence text (no byte below 0x21 but ``\\n``, no ``>``).  Every byte is
below 0x80 (str.rstrip and the byte oracle differ above it).
"""

from __future__ import annotations

import functools
import hashlib
import io

import numpy as np

# The internal sizes of kman_amd/csrc/parse.hip: PB (bytes per thread chunk),
# PTILE (PT * PB, bytes per tile) and SCAN_T (tiles per block of the
# two-level tile scan: a block boundary every SCAN_T * PTILE bytes).
CHUNK = 64
TILE = 16384
BLOCK = 1024 * TILE

EDGES = [63, 64, 65, TILE - 1, TILE, TILE + 1, TILE + 63, TILE + 64, TILE + 65, 2 * TILE - 1, 2 * TILE]
TILE_EDGES = [x for x in EDGES if x % TILE == 0]
WS_EDGES = [64, TILE, TILE + 64]
LETTERS = b"ACGTacgtN"
LF, CR, GT = 0x0A, 0x0D, 0x3E

FAMILIES = ("gt_at", "hdr_tail", "crlf_at", "blank_at", "ws_run", "long_hdr", "pre_junk", "empty_recs", "gt_inside",
            "eof_at", "loader")
LARGE_NAMES = ("big_gt_block_m1", "big_gt_block", "big_gt_block_p1", "big_hdr_spans_block", "big_pre_block",
               "big_crlf_block_no_hdr_after")


# ------------------------------------------------------------ the statement


def _walk(text: bytes):
    """[title, [sequence lines]] per record, the lines as the reference's
    text-mode file yields them (universal newlines)."""
    fh = io.TextIOWrapper(io.BytesIO(text), encoding="latin-1", newline=None)
    recs = []
    for line in fh:
        if line.startswith(">"):
            recs.append([line[1:].rstrip(), []])
        elif recs:
            recs[-1][1].append(line.rstrip())
    return recs


def line_starts(text: bytes) -> np.ndarray:
    """bool per byte: the byte starts a line (after ``\\n``, after a ``\\r``
    that no ``\\n`` follows, and byte 0)."""
    b = np.frombuffer(text, dtype=np.uint8)
    ls = np.zeros(len(b), dtype=bool)
    if len(b):
        ls[0] = True
        ls[1:] = (b[:-1] == LF) | ((b[:-1] == CR) & (b[1:] != LF))
    return ls


def header_offsets(text: bytes) -> np.ndarray:
    b = np.frombuffer(text, dtype=np.uint8)
    return np.nonzero(line_starts(text) & (b == GT))[0].astype(np.uint64)


def statement(text: bytes):
    """-> (records, header_offsets): records as (title, cleaned sequence)
    bytes pairs, and the byte offset of every header's ``>``.  AssertionError
    on a text without a header line."""
    recs = _walk(text)
    if not recs:
        raise AssertionError("premature end of file or empty file")
    out = [(t.encode("latin-1"), "".join(s).replace(" ", "").replace("\r", "").encode("latin-1")) for t, s in recs]
    return out, header_offsets(text)


def reference_loops(text: bytes) -> bool:
    """A record after the first without any sequence line: the reference's
    parser yields it again and again (tests/golden/inputs.py), so such a text
    is not pinned to it."""
    return any(not lines for _, lines in _walk(text)[1:])


def digest(records) -> str:
    """sha256 over the titles and cleaned sequences, each length-prefixed."""
    h = hashlib.sha256()
    for t, s in records:
        h.update(b"%d:%d:" % (len(t), len(s)))
        h.update(t)
        h.update(s)
    return h.hexdigest()


def plain_tile(text: bytes, t: int) -> bool:
    """Tile t is whole and every byte of it is ``\\n`` or >= 0x21 and no ``>``
    (so each of its 64-byte chunks passes the parser's fast test)."""
    b = np.frombuffer(text, dtype=np.uint8)[t * TILE:(t + 1) * TILE]
    return len(b) == TILE and bool(np.all(((b >= 0x21) | (b == LF)) & (b != GT)))


# ---------------------------------------------------------------- builders


@functools.lru_cache(maxsize=None)
def _pool(width: int, size: int) -> np.ndarray:
    rng = np.random.default_rng(1000 + width)
    a = rng.choice(np.frombuffer(LETTERS, np.uint8), size, p=[.24, .24, .24, .24, .01, .01, .01, .005, .005])
    a[width::width + 1] = LF
    return a


def seq_text(rng, n: int, width: int = 61, end_nl: bool = True, big: bool = False) -> bytes:
    """Exactly n bytes of sequence lines, `width` letters each, starting at a
    line start; the last byte is ``\\n`` (no empty line before it), or a
    letter when not end_nl."""
    if n <= 0:
        return b""
    pool = _pool(width, (BLOCK + (2 << 20)) if big else (1 << 18))
    off = int(rng.integers(0, 64)) * (width + 1)
    a = pool[off:off + n].copy()
    assert len(a) == n
    if end_nl:
        a[-1] = LF
        if n >= 2 and a[-2] == LF:
            a[-2] = ord("A")
    elif a[-1] == LF:
        a[-1] = ord("C")
    return a.tobytes()


HEAD = b">r0 first record\n"


def _tail(rng, start: int, width: int, big: bool = False) -> bytes:
    """Sequence lines from `start` through the end of its tile and 2037 bytes
    more, the last 100 of them a record of their own."""
    total = (start // TILE + 1) * TILE + 2037
    return seq_text(rng, total - 100 - start, width, big=big) + b">tail t\n" + seq_text(rng, 92, width)


def _around(rng, X: int, mid: bytes, back: int = 0, open_: bool = False, width: int = 61, tail: bool = True,
            head: bytes = HEAD) -> bytes:
    """head, sequence lines, then `mid` with mid[back] at byte X (`open_`: the
    byte before mid is a letter, not a line end), then _tail."""
    start = X - back
    pre = head + seq_text(rng, start - len(head), width, end_nl=not open_)
    assert len(pre) == start and start - len(head) >= 1
    text = pre + mid
    if tail:
        text += _tail(rng, len(text), width)
    return text


def _fast(text: bytes, X: int):
    """The premise of a fast-path case at a tile edge: the tile that starts
    at X is plain sequence text."""
    return [X // TILE] if X % TILE == 0 and plain_tile(text, X // TILE) else None


def _junk(rng, n: int) -> bytes:
    """Exactly n bytes before the first header, ending in ``\\n``: comments,
    blank lines, sequence-looking lines, ``>`` inside a line."""
    kinds = [b"; a comment line\n", b"\n", None, b"xx>yy\n", b"ACGT>ACGT\n", b"\r\n", None, b"# note\r", None, b" \t\n"]
    out, left, i = [], n, 0
    while left > 130:
        ln = kinds[i % len(kinds)]
        if ln is None:
            ln = seq_text(rng, 62, 61)
        out.append(ln)
        left -= len(ln)
        i += 1
    if left:
        out.append(seq_text(rng, left, 200))
    text = b"".join(out)
    assert len(text) == n
    return text


def _title(rng, n: int, ws: bool) -> bytes:
    t = bytearray(rng.choice(np.frombuffer(b"ACGTNacgtnXYZ", np.uint8), n).tobytes())
    if ws:
        t[1:3] = b" \t"
    return bytes(t)


def _ws(rng, L: int, exotic: bool) -> bytes:
    ab = b" \t\x0b\x0c\x1c\x1f" if exotic else b" \t"
    r = bytearray(rng.choice(np.frombuffer(ab, np.uint8), L).tobytes())
    r[0] = 9  # the chunk where the run starts holds a byte that rstrip decides
    r[-1] = 0x20 if L == 2 else (0x0b if exotic else 9)
    return bytes(r)


@functools.lru_cache(maxsize=None)
def small_cases() -> dict:
    rng = np.random.default_rng(20250)
    out = {}

    def add(name, text, **meta):
        assert name not in out and max(text) < 0x80
        out[name] = (text, meta)

    def width():
        return int(rng.choice([61, 80]))

    for X in EDGES:
        t = _around(rng, X, b">g%d name here\n" % X, width=width())
        add("gt_at_%d" % X, t, family="gt_at", at=X, byte=">", before="\n")

    for X in TILE_EDGES:
        for h in (1, 2, 9, 70):
            for d in (0, 1, 7, 8, 9, 64, 65):
                for ws in (False, True):
                    n = h - 1 + d
                    if ws and n < 3:
                        continue
                    t = _around(rng, X, b">" + _title(rng, n, ws) + b"\n", back=h, width=width())
                    # (the title's space and tab sit before X only when h >= 9)
                    add("hdr_tail_%d_h%d_d%d_%s" % (X, h, d, "ws" if ws else "letters"), t, family="hdr_tail",
                        at=X - h, byte=">", before="\n", last=X - 1 + d, fast_tiles=_fast(t, X))

    for X in EDGES:
        w = width()
        t = _around(rng, X, b"\r\n", back=1, open_=True, width=w)
        add("crlf_at_%d" % X, t, family="crlf_at", at=X, byte="\n", before="\r", fast_tiles=_fast(t, X))
        t = _around(rng, X, b"\r", back=1, open_=True, width=w)
        add("cr_base_at_%d" % X, t, family="crlf_at", at=X, byte="base", before="\r", fast_tiles=_fast(t, X))
        t = _around(rng, X, b"\r>c%d after a lone cr\n" % X, back=1, open_=True, width=w)
        add("cr_gt_at_%d" % X, t, family="crlf_at", at=X, byte=">", before="\r")
        for back in (1, 2, 3):
            t = _around(rng, X, b"\r\n\r\n", back=back, open_=True, width=w)
            add("crlfcrlf_b%d_at_%d" % (back, X), t, family="crlf_at", at=X, byte="\r\n\r\n"[back:back + 1],
                before="\r\n\r\n"[back - 1:back], fast_tiles=_fast(t, X) if back != 2 else None)

    for X in EDGES:
        for n, back, mid in ((3, 1, b"\n\n\n"), (4, 2, b"\n\n\n\n"), (5, 3, b"\n\r\n\r\r\n\n")):
            t = _around(rng, X, mid, back=back, width=width())
            add("blank%d_at_%d" % (n, X), t, family="blank_at", at=X, byte=mid[back:back + 1].decode(),
                before=mid[back - 1:back].decode(), fast_tiles=_fast(t, X) if n < 5 else None)

    for X in WS_EDGES:
        for L in (2, 65, 130, TILE + 10):
            for exotic in (False, True):
                run = _ws(rng, L, exotic)
                for end in ("nl", "base", "eof"):
                    mid = run + (b"\n" if end == "nl" else b"")
                    t = _around(rng, X, mid, back=3, open_=True, width=width(), tail=end != "eof")
                    add("ws_run_%d_L%d_%s_%s" % (X, L, "exotic" if exotic else "plain", end), t, family="ws_run",
                        at=X - 3, byte="\t", before="base", run=L, end=end)

    for space in (False, True):
        title = bytearray(_title(rng, 3 * TILE + 17, False))
        if space:
            title[len(title) // 2] = 0x20
        t = _around(rng, 100, b">" + bytes(title) + b"\n", width=61, tail=False)
        t += seq_text(rng, 4 * TILE - 5 - len(t), 61)
        add("long_hdr_space" if space else "long_hdr_letters", t, family="long_hdr", at=100, byte=">", before="\n",
            last=100 + 3 * TILE + 17, fast_tiles=[2] if space else [1, 2])
    t = _around(rng, 100, b">" + _title(rng, 4 * TILE - 102, False) + b"\n", width=80, tail=False)
    t += seq_text(rng, 1000, 80)
    add("long_hdr_ends_4tile_m1", t, family="long_hdr", at=4 * TILE - 1, byte="\n", before=None, fast_tiles=[1, 2, 3])

    for X in EDGES + [2 * TILE + 100]:
        t = _junk(rng, X) + b">p%d after the junk\n" % X
        t += _tail(rng, len(t), width())
        add("pre_junk_%d" % X, t, family="pre_junk", at=X, byte=">", before="\n")

    for X in EDGES:
        for term in (b"\n", b"\r"):
            mid = b"".join(b">e%d" % i + term for i in range(10))
            t = _around(rng, X, mid, back=20, width=width())
            add("empty_recs_%s_at_%d" % ("lf" if term == b"\n" else "cr", X), t, family="empty_recs", at=X, byte=">",
                before=term.decode())
    t = _around(rng, TILE, b"".join(b">h%05d\n" % i for i in range(TILE // 8)), width=61)
    add("empty_recs_header_tile", t, family="empty_recs", at=TILE, byte=">", before="\n", only_tile=1)
    blank = b"".join([b"\n", b"\r\n", b" ", b"  \n"][i] for i in rng.integers(0, 4, TILE))[:TILE - 1] + b"\n"
    t = _around(rng, TILE, blank, width=80)
    add("empty_recs_blank_tile", t, family="empty_recs", at=TILE, byte=None, before="\n", only_tile=1)

    for X in EDGES:
        t = _around(rng, X, b">", open_=True, width=width())
        add("gt_inside_%d" % X, t, family="gt_inside", at=X, byte=">", before="base")

    for X in (64, 128, TILE, TILE + 1, 2 * TILE):
        w = width()
        n = X - len(HEAD)
        for end, text in (("base", HEAD + seq_text(rng, n, w, end_nl=False)),
                          ("nl", HEAD + seq_text(rng, n, w)),
                          ("cr", HEAD + seq_text(rng, n - 1, w, end_nl=False) + b"\r"),
                          ("crlf", HEAD + seq_text(rng, n - 2, w, end_nl=False) + b"\r\n"),
                          ("gtname", HEAD + seq_text(rng, n - 5, w) + b">last")):
            add("eof_at_%d_%s" % (X, end), text, family="eof_at", at=X - 1, byte=None, before=None, length=X, end=end)
    add("eof_lone_gt_last_tile", HEAD + seq_text(rng, TILE - len(HEAD), 61) + b">", family="eof_at", at=TILE, byte=">",
        before="\n", length=TILE + 1, end="gt")

    # for the chunked loader: a header line that ends at byte A, then blank
    # lines up to byte 2 A and beyond, then the record's bases
    pre = HEAD + seq_text(rng, 62, 61) + b">h1 blank lines follow\n"
    t = pre + b"\n" * (len(pre) + 9) + seq_text(rng, 600, 61) + b">h2\n" + seq_text(rng, 130, 61)
    add("loader_blank_chunk", t, family="loader", at=len(pre), byte="\n", before="\n", chunk=len(pre))
    return out


def _big_tail(rng, start: int) -> bytes:
    total = BLOCK + (1 << 20) + 4321
    return seq_text(rng, total - 100 - start, 80, big=True) + b">tail t\n" + seq_text(rng, 92, 80)


@functools.lru_cache(maxsize=2)
def large_case(name: str):
    """One text of just over 1024 tiles (17 MiB): built when asked for."""
    rng = np.random.default_rng(LARGE_NAMES.index(name))
    if name.startswith("big_gt_block"):
        X = BLOCK + {"big_gt_block_m1": -1, "big_gt_block": 0, "big_gt_block_p1": 1}[name]
        t = HEAD + seq_text(rng, X - len(HEAD), 80, big=True) + b">g at the block edge\n"
        return t + _big_tail(rng, len(t)), dict(family="large", at=X, byte=">", before="\n")
    if name == "big_hdr_spans_block":
        X = BLOCK - 40
        t = HEAD + seq_text(rng, X - len(HEAD), 61, big=True) + b">" + _title(rng, 100, False) + b"\n"
        return t + _big_tail(rng, len(t)), dict(family="large", at=X, byte=">", before="\n", last=X + 100)
    if name == "big_pre_block":
        X = BLOCK + TILE + 77
        a = np.frombuffer(seq_text(rng, X, 61, big=True), np.uint8).copy()
        a[0] = ord(";")
        a[62 * 1000 + 5::62 * 1000] = GT  # `>` inside every 1000th line, never at a line start
        t = a.tobytes() + b">first header after the block\n"
        return t + _big_tail(rng, len(t)), dict(family="large", at=X, byte=">", before="\n", first_header=X)
    if name == "big_crlf_block_no_hdr_after":
        t = HEAD + seq_text(rng, BLOCK - 1 - len(HEAD), 80, end_nl=False, big=True) + b"\r\n"
        t += seq_text(rng, (1 << 20) + 4321, 80, big=True)
        return t, dict(family="large", at=BLOCK, byte="\n", before="\r", no_header_from=BLOCK)
    raise KeyError(name)


def cases() -> dict:
    """Every case, the large ones included (about 100 MB of text)."""
    out = dict(small_cases())
    for name in LARGE_NAMES:
        out[name] = large_case(name)
    return out
