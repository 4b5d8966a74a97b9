"""Code arrays that put every event of the k <= 32 window kernels on a tile,
thread or pad edge (extract_kernel, count_kernel, kmer_hist_kernel in
kman_amd/csrc/extract.hip; the fused extract_pass in sort.hip; load_codes,
store_codes and roll in kmer.h / rollfast.h).  numpy and Python only.

A case is built without a parser: a list of record sequences goes through
np_oracle.codes_of, 64 pad codes of value 4 follow (include/kman.h,
kman_parse_fasta), and the raw-code family then edits single codes.

Two statements of the expected stream:
  1. np_oracle.stream_kmers on the case's records (the reference's windows);
  2. code_stream() here, from the codes alone: window i is valid iff none of
     its k codes has bit 2 set (not ACGT) and no code after its first has
     bit 3 set (record start); key = 2 bits per base, first base most
     significant; rc key = complement, reversed; canonical = min of the two;
     mixed = np_oracle.mix_keys of the canonical key.
test_extract_cases_cpu.py asserts that they agree and that every family holds
what it promises; test_gpu_extract_edges.py runs the entry points on them."""

from __future__ import annotations

import functools

import numpy as np

import np_oracle

# Window starts per tile and per thread, and the threads of a block:
#   extract_kernel  ET = 256 (extract.hip `constexpr int ET = 256`); EI = 16,
#                   or 8 with -r alone (dispatch_extract: launch_extract<8, true, 0, P>)
#   count_kernel    count_kernel<16> (kman_count_kmers)
#   kmer_hist       `const int EI = 16` (kman_kmer_hist)
#   extract_pass    XT = 512 (sort.hip `constexpr int XT = 512`); WIN = XT * (rc ? 8 : 16)
#                   (kman_extract_sorted `const uint64_t WIN`)
TILE_EXTRACT, TILE_EXTRACT_RC = 256 * 16, 256 * 8
TILE_COUNT = TILE_HIST = 256 * 16
WIN_PASS, WIN_PASS_RC = 512 * 16, 512 * 8
WAVE = 64          # threads of a wave: it spans 64 * (8 or 16) window starts
COUNT_GRID = 4096  # kman_count_kmers `n_tiles < 4096 ? n_tiles : 4096`
NSEG = 8           # sort.hip `constexpr int NSEG = 8`: kman_seg_fit gives at most this
PAD = 64

E = (2048, 4096, 8192, 16384)
K = (2, 3, 5, 9, 16, 17, 25, 31, 32)
K_SUB = (2, 21, 32)
K_B = tuple(sorted(set(K) | set(K_SUB)))  # family B: K and the subset's 21
VARIANTS = ("fwd", "rc", "canon", "mixed")
FAMILIES = "ABCDEFGH"


def deltas(k: int):
    """Family B: the event sits at e + d."""
    return tuple(dict.fromkeys((-k, -k + 1, -16, -8, -1, 0, 1, 7, 8, 15, 16, k - 2, k - 1)))


class Case:
    """codes: n_bases codes + 64 pad codes (read-only); records: the
    (title, sequence) list whose stream_kmers is the expected stream (for a
    raw-code case, the records of its twin with codes 4 and 12)."""

    def __init__(self, name, family, k, records, codes=None, **meta):
        self.name, self.family, self.k, self.records, self.meta = name, family, k, records, meta
        if codes is None:
            codes = np_oracle.codes_of(records)[0]
        self.n_bases = len(codes)
        self.codes = np.concatenate([codes, np.full(PAD, 4, np.uint8)])
        self.codes.setflags(write=False)
        assert self.n_bases == sum(len(s) for _, s in records)

    def expected(self, variant: str, k: int = 0):
        return record_stream(self.records, k or self.k, variant)

    def __repr__(self):
        return "Case(%s)" % self.name


# ------------------------------------------------------------ the statements


def record_stream(records, k: int, variant: str):
    """Statement 1 -> (keys, pos), both uint64, in stream order."""
    keys, pos = np_oracle.stream_kmers(records, k, rc=variant == "rc", canonical=variant in ("canon", "mixed"))
    if variant == "mixed":
        keys = np_oracle.mix_keys(keys, k)
    return keys, pos


def code_windows(codes, n_bases: int, k: int):
    """Statement 2, the rule of every window i in [0, n_bases - k], one offset
    j of the window per step: -> (starts of the valid windows, forward keys,
    rc keys)."""
    c = np.asarray(codes[:n_bases])
    nw = n_bases - k + 1
    if nw <= 0:
        z = np.zeros(0, np.uint64)
        return np.zeros(0, np.int64), z, z
    ok = np.ones(nw, bool)
    f = np.zeros(nw, np.uint64)
    r = np.zeros(nw, np.uint64)
    for j in range(k):
        cj = c[j:j + nw]
        ok &= (cj & 4) == 0
        if j:
            ok &= (cj & 8) == 0
        b = (cj & 3).astype(np.uint64)
        f |= b << np.uint64(2 * (k - 1 - j))
        r |= (np.uint64(3) - b) << np.uint64(2 * j)
    s = np.nonzero(ok)[0]
    return s, f[s], r[s]


def code_stream(codes, n_bases: int, k: int, variant: str, windows=None):
    """Statement 2 -> (keys, pos) as record_stream's (windows: code_windows'
    answer, when the caller has it)."""
    s, f, r = windows or code_windows(codes, n_bases, k)
    gp = s.astype(np.uint64) << np.uint64(1)
    if variant == "fwd":
        return f, gp
    if variant == "rc":
        keys, pos = np.empty(2 * len(s), np.uint64), np.empty(2 * len(s), np.uint64)
        keys[0::2], keys[1::2] = f, r
        pos[0::2], pos[1::2] = gp, gp | np.uint64(1)
        return keys, pos
    keys = np.minimum(f, r)
    return (np_oracle.mix_keys(keys, k) if variant == "mixed" else keys), gp


def code_stream_plain(codes, n_bases: int, k: int):
    """The same rule with Python integers, window by window (small cases):
    -> list of (start, forward key, rc key)."""
    out = []
    for i in range(n_bases - k + 1):
        w = [int(x) for x in codes[i:i + k]]
        if any(x & 4 for x in w) or any(x & 8 for x in w[1:]):
            continue
        f = r = 0
        for j, x in enumerate(w):
            f = (f << 2) | (x & 3)
            r |= (3 - (x & 3)) << (2 * j)
        out.append((i, f, r))
    return out


def tile_counts(pos, n_bases: int, tile: int):
    """Valid windows per tile of `tile` window starts (forward pos)."""
    nt = -(-n_bases // tile)
    return np.bincount((pos >> np.uint64(1)).astype(np.int64) // tile, minlength=nt)


# ----------------------------------------------------------------- builders


def _acgt(seed, n: int) -> bytes:
    return np.frombuffer(b"ACGT", np.uint8)[np.random.default_rng(seed).integers(0, 4, n)].tobytes()


def _recs(*seqs):
    return [(b"r%d" % i, bytes(s)) for i, s in enumerate(seqs)]


def _split(seq: bytes, *cuts):
    """The record sequences of `seq` with a record start at every cut."""
    at = [0] + sorted(c for c in set(cuts) if 0 < c < len(seq)) + [len(seq)]
    return [seq[a:b] for a, b in zip(at, at[1:])]


def _with_n(seq: bytes, *ps):
    b = bytearray(seq)
    for p in ps:
        b[p] = ord("N")
    return bytes(b)


@functools.lru_cache(maxsize=None)
def base_record(e: int) -> bytes:
    """Family B's event-free record: random ACGT, two 4096-tiles past e."""
    return _acgt(1000 + e, e + 2 * 4096 + 37)


def family_a(ks=K):
    for k in ks:
        lens = [(n, "n%d" % n) for n in sorted({1, k - 1, k, k + 1})]
        lens += [(e + d, "e%d%+d" % (e, d)) for e in E for d in sorted({-1, 0, 1, k - 2, k - 1, k})]
        for n, tag in lens:
            yield Case("a_k%d_%s" % (k, tag), "A", k, _recs(_acgt(n, n)), n=n)
    for n in A_INTERVAL:
        yield Case("a_k21_pad_%d" % n, "A", 21, _recs(_acgt(n, n)), n=n, interval=True)


# every residue of n_bases and of n_bases + 64 mod 16 on both sides of the point
# where the last vectors of a 4096-tile cross n_bases + 64
A_INTERVAL = tuple(range(4096 - 80, 4096 + 16 + 1))


def event_case(family, k, e, d, kind, name=None):
    """One event at p = e + d in base_record(e): kind "n" (a not-ACGT code),
    "start" (a record start), "nstart" (a record start on a not-ACGT code),
    "n_then_start" (N at p, start at p + 1), "start_then_n"."""
    p, seq = e + d, base_record(e)
    if kind == "n":
        recs = [_with_n(seq, p)]
    elif kind == "start":
        recs = _split(seq, p)
    elif kind == "nstart":
        recs = _split(_with_n(seq, p), p)
    elif kind == "n_then_start":
        recs = _split(_with_n(seq, p), p + 1)
    else:
        assert kind == "start_then_n"
        recs = _split(_with_n(seq, p + 1), p)
    return Case(name or "%s_k%d_e%d_d%+d_%s" % (family.lower(), k, e, d, kind), family, k, _recs(*recs), e=e, d=d, p=p,
                kind=kind)


def gone(case: Case):
    """The window starts an event case loses against base_record(e)."""
    k, p, kind = case.k, case.meta["p"], case.meta["kind"]
    lo, hi = {"n": (p - k + 1, p), "start": (p - k + 1, p - 1), "nstart": (p - k + 1, p),
              "n_then_start": (p - k + 1, p), "start_then_n": (p - k + 1, p + 1)}[kind]
    last = len(base_record(case.meta["e"])) - k
    return set(range(max(lo, 0), min(hi, last) + 1))


def family_b(ks=K_B, es=E, both=True):
    for k in ks:
        for e in es:
            for d in deltas(k):
                for kind in ("n", "start"):
                    yield event_case("B", k, e, d, kind)
            if both and k in K_SUB:
                yield event_case("B", k, e, -1, "n_then_start")
                yield event_case("B", k, e, -1, "start_then_n")


RAW_N, RAW_START = (5, 6, 7), (12, 13, 14, 15)


def family_c(ks=(5, 32), es=E):
    """Family B with the not-ACGT code drawn from 5, 6, 7 and record starts on
    the not-ACGT codes 12 .. 15: the expected stream is that of codes 4 and 12."""
    i = 0
    for k in ks:
        for e in es:
            for d in deltas(k):
                i += 1
                for kind in ("n", "nstart"):
                    twin = event_case("C", k, e, d, kind)
                    codes = twin.codes[:twin.n_bases].copy()
                    raw = (RAW_N if kind == "n" else RAW_START)[i % (3 if kind == "n" else 4)]
                    assert codes[twin.meta["p"]] == (4 if kind == "n" else 12)
                    codes[twin.meta["p"]] = raw
                    yield Case("%s_raw%d" % (twin.name, raw), "C", k, twin.records, codes, raw=raw, **twin.meta)


def family_d(ks=K, es=(2048, 4096, 8192)):
    """Records of length k (one window), k - 1 (none) and 1 from 3k before e to
    3k after it, between two long records."""
    for k in ks:
        for e in es:
            rng = np.random.default_rng(77 * k + e)
            seqs, at = [_acgt(e + k, e - 3 * k)], e - 3 * k
            while at < e + 3 * k:
                n = (k, k - 1, 1)[int(rng.integers(0, 3))]
                seqs.append(_acgt(at, n))
                at += n
            seqs.append(_acgt(e - k, 4096 + 5))
            yield Case("d_k%d_e%d" % (k, e), "D", k, _recs(*seqs), e=e, run=(e - 3 * k, at))


E_TILES = (2048, 4096, 8192)
# (tile, window starts of a wave): extract_kernel -r, extract_kernel / count /
# hist, extract_pass -r, extract_pass
E_WAVES = ((2048, 512), (4096, 1024), (4096, 512), (8192, 1024))


def _from_valid(n: int, spans, seed):
    """A record of n codes, N everywhere but ACGT on the spans [a, b)."""
    b = bytearray(b"N" * n)
    for a, z in spans:
        b[a:z] = _acgt(seed + a, z - a)
    return bytes(b)


def family_e(ks=K_SUB):
    for k in ks:
        for T in E_TILES:
            # full, N, N, one window at the last start, one at the first start, N, a short tail
            tail = 100 + k
            seq = _from_valid(6 * T + tail, [(0, T), (4 * T - 1, 4 * T + k), (6 * T, 6 * T + tail)], T + k)
            want = [T - k + 1, 0, 0, 1, 1, 0, tail - k + 1]
            yield Case("e_k%d_sparse_t%d" % (k, T), "E", k, _recs(*_split(seq, 6 * T)), tile=T, counts=want,
                       single={3: 4 * T - 1, 4: 4 * T})
        yield Case("e_k%d_all_n" % k, "E", k, _recs(b"N" * (3 * 8192)), tile=8192, counts=[0, 0, 0])
        for T, W in E_WAVES:
            waves = [(3 * t + 1) % (T // W) for t in range(5)]
            spans = [(t * T + w * W, t * T + (w + 1) * W + k - 1) for t, w in enumerate(waves)]
            yield Case("e_k%d_wave_t%d_w%d" % (k, T, W), "E", k, _recs(_from_valid(5 * T, spans, W + k)), tile=T,
                       counts=[W] * 5, wave=W, waves=waves)


def _rc_text(s: bytes) -> bytes:
    return s.translate(bytes.maketrans(b"ACGT", b"TGCA"))[::-1]


def family_f(ks=(31, 32)):
    n = 4096 + 200
    for k in ks:
        yield Case("f_k%d_poly_a" % k, "F", k, _recs(b"A" * n), kind="poly_a")
        yield Case("f_k%d_poly_t" % k, "F", k, _recs(b"T" * n), kind="poly_t")
        yield Case("f_k%d_poly_acgt" % k, "F", k, _recs(b"A" * n, b"C" * 100, b"G" * 100, b"T" * n, b"ACGT" * (n // 4)),
                   kind="poly_acgt")
        # every window of even length reads the same on both strands
        yield Case("f_k%d_palindrome" % k, "F", k, _recs(b"AT" * (n // 2), b"CG" * 300), kind="palindrome")
        # random: forward < rc and forward > rc change places about every other window
        yield Case("f_k%d_alternate" % k, "F", k, _recs(_acgt(31 + k, n)), kind="alternate")


G_COUNTS = (1, 2, 7, 8, 9, 17)


def family_g():
    """All-ACGT inputs of G_COUNTS tiles of kman_extract_sorted's pass, below,
    at and above its 8 window segments; rc: the case is for the -r tile."""
    for win in (WIN_PASS, WIN_PASS_RC):
        for c in G_COUNTS:
            n = (c - 1) * win + 777
            seq = _acgt(win + c, n)
            yield Case("g_win%d_c%d" % (win, c), "G", 0, _recs(*_split(seq, n // 3)), win=win, tiles=c,
                       rc=win == WIN_PASS_RC)


H_TILES = 4099
H_BASES = H_TILES * 4096 - 5


@functools.lru_cache(maxsize=1)
def family_h() -> Case:
    """4099 tiles of 4096 codes against count_kernel's 4096 blocks and the
    persistent grids: 300 stretches of N, each followed by about 7000 ACGT
    codes (about 2 M valid windows), the ACGT part a record of its own in
    every other one."""
    rng = np.random.default_rng(4099)
    units, seqs, left = 300, [], H_BASES
    for u in range(units):
        n = left if u == units - 1 else H_BASES // units
        left -= n
        a = int(rng.integers(6000, 8000))
        filler, run = b"N" * (n - a), _acgt(9000 + u, a)
        seqs += [filler + run] if u % 2 == 0 else [filler, run]
    return Case("h_4099_tiles", "H", 21, _recs(*seqs), tiles=H_TILES)


def small_cases():
    """Every case of A-G, in family order."""
    for fam in (family_a, family_b, family_c, family_d, family_e, family_f, family_g):
        yield from fam()


def fasta_text(case: Case, width: int = 70) -> bytes:
    """The case's records as FASTA, lines of `width`."""
    out = []
    for t, s in case.records:
        out.append(b">" + t)
        out += [s[i:i + width] for i in range(0, len(s), width)]
    return b"\n".join(out) + b"\n"
