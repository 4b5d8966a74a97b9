// fastq.hip — strict four-line FASTQ text -> cleaned base codes + record table,
// on the GPU, in the kman_parse_fasta output contract (include/kman.h).
//
// Lines are split as parse.hip splits them ("\n", "\r\n" and a lone "\r" end a
// line).  Trailing empty lines are dropped and the rest is padded with empty
// lines to a multiple of four; line 4r is record r's '@' header, 4r + 1 its
// sequence, 4r + 2 the '+' separator and 4r + 3 the quality, which must be as
// long as line 4r + 1.  The sequence line is cleaned as a FASTA sequence line
// (right-stripped, ' ' and '\r' removed, swar.h's codes4 per byte).
//
// The only non-local fact of a byte is its line kind = (line starts up to and
// including it - 1) mod 4.  A chunk's summary is its line count and, for each
// of the four residues j mod 4 of the chunk-local inclusive line count j, the
// content bytes that sit at that residue; two summaries compose by rotating
// the second by the first's line count.  The file is parsed with parse.hip's
// skeleton: reduce over 16 KiB tiles -> two-level tile scan -> emit.  There is
// no plain-text fast path (every tile holds headers and quality bytes), so the
// one path works on bit masks built with SWAR byte tests and never indexes the
// chunk's bytes at run time.
//
// The emit pass also writes every line's start offset; a per-record kernel
// compares the lengths of lines 2 and 4 and tests the first bytes of lines 1
// and 3 from those offsets (no thread walks a line), and the smallest
// offending (record, rule) leaves the device as one word.
//
// Memory traffic: the text is read twice, about half of it is written as
// codes, 8 B per line and 16 B per record of tables: ~2.7 B per input byte for
// 150-base reads.
//
// A quality threshold (kman_parse_fastq_q) adds one pass, fq_qmask, after the
// validation: a kept sequence byte whose quality byte (same column, two lines
// on) is below the threshold has its code turned into that of an 'N'.  See the
// kernel for its traffic.
#include "common.h"
#include "swar.h"

namespace {

constexpr int PT = 256;           // threads per tile
constexpr int PB = 64;            // bytes per thread
constexpr int PTILE = PT * PB;    // 16 KiB per tile
constexpr int SCAN_T = 1024;      // tiles per block of the two-level tile scan

// k[r]: content bytes whose chunk-local inclusive line count j has j mod 4 == r
// last_ne: 1 + the local index of the last non-empty line start (0: none)
struct Lq {
    uint32_t lines;
    uint32_t k[4];
    uint32_t last_ne;
};
struct Lq64 {
    uint64_t lines;
    uint64_t k[4];
    uint64_t last_ne;
};

// select without runtime array indexing (which would go to scratch)
template <typename T>
KMAN_DEV T sel4(const T (&a)[4], uint32_t s) {
    return s == 0 ? a[0] : (s == 1 ? a[1] : (s == 2 ? a[2] : a[3]));
}

template <typename Q>
struct ComposeLq {
    KMAN_DEV Q operator()(const Q &a, const Q &b) const {
        Q r;
        const uint32_t s = (uint32_t)a.lines & 3u;
        r.lines = a.lines + b.lines;
#pragma unroll
        for (uint32_t i = 0; i < 4; i++) r.k[i] = a.k[i] + sel4(b.k, (i - s) & 3u);
        r.last_ne = b.last_ne ? a.lines + b.last_ne : a.last_ne;
        return r;
    }
};

template <typename Q>
KMAN_DEV Q lq_id() {
    Q q;
    q.lines = 0;
    q.k[0] = q.k[1] = q.k[2] = q.k[3] = 0;
    q.last_ne = 0;
    return q;
}

// (SWAR byte tests on 4 packed bytes, as swar.h's: 0x80 in every byte that passes)
// bytes below c (c <= 0x80)
KMAN_DEV uint32_t lt_bytes(uint32_t w, uint32_t c) {
    return ~((w & 0x7f7f7f7fu) + (0x80u - c) * 0x01010101u) & ~w & 0x80808080u;
}
// bytes below c, unsigned, for any c in 1..255
KMAN_DEV uint32_t lt_bytes_u8(uint32_t w, uint32_t c) {
    const bool hi = c > 0x80u;  // (then every byte below 0x80 passes, the others by their low 7 bits)
    const uint32_t lo7 = ~((w & 0x7f7f7f7fu) + (0x80u - (hi ? c - 0x80u : c)) * 0x01010101u) & 0x80808080u;
    return hi ? ((~w & 0x80808080u) | (lo7 & w)) : (lo7 & ~w);
}
// bit i = xor of bits 0..i
KMAN_DEV uint64_t prefix_xor(uint64_t x) {
    x ^= x << 1;
    x ^= x << 2;
    x ^= x << 4;
    x ^= x << 8;
    x ^= x << 16;
    x ^= x << 32;
    return x;
}

// A thread's 64-byte chunk of the text, reduced to bit masks (bit i = byte i).
struct Chunk {
    uint32_t w[PB / 4];
    uint64_t ls;    // byte starts a line (universal newlines)
    uint64_t ne;    // ... a non-empty line
    uint64_t keep;  // content byte (not a terminator, not ' ', not trailing whitespace)
};

KMAN_DEV void load_chunk(const uint8_t *text, uint64_t n, uint64_t pos, Chunk &ch) {
    const int cnt = pos < n ? (int)((n - pos) < (uint64_t)PB ? (n - pos) : (uint64_t)PB) : 0;
    if (cnt == PB) {
        const uint4 *p = reinterpret_cast<const uint4 *>(text + pos);
#pragma unroll
        for (int v = 0; v < PB / 16; v++) {
            const uint4 x = p[v];
            ch.w[4 * v + 0] = x.x;
            ch.w[4 * v + 1] = x.y;
            ch.w[4 * v + 2] = x.z;
            ch.w[4 * v + 3] = x.w;
        }
    } else {
#pragma unroll
        for (int q = 0; q < PB / 4; q++) {
            uint32_t v = 0;
#pragma unroll
            for (int b = 0; b < 4; b++) {
                const int i = 4 * q + b;
                v |= (i < cnt ? (uint32_t)text[pos + i] : 0u) << (8 * b);
            }
            ch.w[q] = v;
        }
    }
    // position 0 starts a line; a chunk wholly past the end reads nothing (its
    // byte before may lie past the allocation)
    const uint32_t prev = pos == 0 ? '\n' : (pos <= n ? text[pos - 1] : 0u);
    uint64_t nl = 0, cr = 0, sp = 0;
    uint32_t ctl = 0;  // a byte below 0x20 that is no terminator (rare; zero fill of a tail chunk too)
#pragma unroll
    for (int v = 0; v < PB / 4; v++) {
        const uint32_t w = ch.w[v];
        const uint32_t znl = eq_bytes(w, '\n'), zcr = eq_bytes(w, '\r');
        ctl |= lt_bytes(w, 0x20) & ~(znl | zcr);
        nl |= (uint64_t)hibits4(znl) << (4 * v);
        cr |= (uint64_t)hibits4(zcr) << (4 * v);
        sp |= (uint64_t)hibits4(eq_bytes(w, ' ')) << (4 * v);
    }
    const uint64_t inr = bits_below(cnt);
    const uint64_t term = nl | cr;
    const uint64_t ls = (((nl << 1) | (uint64_t)(prev == '\n')) | (((cr << 1) | (uint64_t)(prev == '\r')) & ~nl)) & inr;
    uint64_t keep = ~(term | sp) & inr;
    if (ctl) {
        // whitespace that str.rstrip() strips only when trailing: \t \v \f \x1c-\x1f
        uint64_t exo = 0;
#pragma unroll
        for (int v = 0; v < PB / 4; v++) {
            const uint32_t w = ch.w[v];
            const uint32_t x = (lt_bytes(w, 14) & ~lt_bytes(w, 9)) | (lt_bytes(w, 0x20) & ~lt_bytes(w, 0x1c));
            exo |= (uint64_t)hibits4(x) << (4 * v);
        }
        exo &= ~term & inr;
        if (exo) {
            // such a byte survives only if a non-whitespace byte follows it in
            // the same line (possibly beyond this chunk)
            const uint64_t nonws = ~(term | sp | exo) & inr;
            const uint64_t stop = term | ~inr;  // (the end of the text ends the line)
            int later = -1;                     // beyond the chunk: not probed yet
            for (uint64_t m = exo; m; m &= m - 1) {
                const int e = __ffsll((unsigned long long)m) - 1;
                const uint64_t after = stop & bits_from(e + 1);
                const int nt = after ? __ffsll((unsigned long long)after) - 1 : 64;
                if (nonws & bits_from(e + 1) & bits_below(nt)) continue;
                if (nt == 64) {
                    if (later < 0) {
                        later = 0;
                        for (uint64_t j = pos + PB; j < n; j++) {
                            const uint32_t c = text[j];
                            if (is_term(c)) break;
                            if (!py_space(c)) {
                                later = 1;
                                break;
                            }
                        }
                    }
                    if (later) continue;
                }
                keep &= ~(1ull << e);
            }
        }
    }
    ch.ls = ls;
    ch.ne = ls & ~term;
    ch.keep = keep;
}

// content bytes at residue r of the chunk-local inclusive line count
KMAN_DEV void residue_masks(const Chunk &ch, uint64_t (&km)[4]) {
    const uint64_t p0 = prefix_xor(ch.ls);         // bit 0 of the count
    const uint64_t p1 = prefix_xor(ch.ls & ~p0);   // bit 1: flips where the count turns even
    km[0] = ch.keep & ~p0 & ~p1;
    km[1] = ch.keep & p0 & ~p1;
    km[2] = ch.keep & ~p0 & p1;
    km[3] = ch.keep & p0 & p1;
}

KMAN_DEV Lq chunk_lq(const Chunk &ch, const uint64_t (&km)[4]) {
    Lq q;
    q.lines = __popcll(ch.ls);
#pragma unroll
    for (int r = 0; r < 4; r++) q.k[r] = __popcll(km[r]);
    q.last_ne = ch.ne ? (uint32_t)__popcll(ch.ls & bits_below(64 - __clzll((unsigned long long)ch.ne))) : 0u;
    return q;
}

__global__ __launch_bounds__(PT) void fq_reduce(const uint8_t *__restrict__ text, uint64_t n,
                                                Lq64 *__restrict__ tiles) {
    __shared__ Lq lds[PT / 64];
    const uint64_t pos = (uint64_t)blockIdx.x * PTILE + (uint64_t)threadIdx.x * PB;
    Lq x;
    {
        Chunk ch;
        load_chunk(text, n, pos, ch);
        uint64_t km[4];
        residue_masks(ch, km);
        x = chunk_lq(ch, km);
    }
    Lq tot;
    block_exclusive_scan<PT>(x, ComposeLq<Lq>(), lq_id<Lq>(), lds, &tot);
    if (threadIdx.x == 0) {
        Lq64 t;
        t.lines = tot.lines;
        for (int r = 0; r < 4; r++) t.k[r] = tot.k[r];
        t.last_ne = tot.last_ne;
        tiles[blockIdx.x] = t;
    }
}

// Tile scan, level 1: SCAN_T tiles per block -> each tile's exclusive prefix
// inside its block, and the block's total.
__global__ __launch_bounds__(SCAN_T) void fq_scan_blocks(const Lq64 *__restrict__ tiles, uint64_t T,
                                                         Lq64 *__restrict__ local, Lq64 *__restrict__ btot) {
    __shared__ Lq64 lds[SCAN_T / 64];
    const uint64_t t = (uint64_t)blockIdx.x * SCAN_T + threadIdx.x;
    const Lq64 id = lq_id<Lq64>();
    const Lq64 x = t < T ? tiles[t] : id;
    Lq64 tot;
    const Lq64 ex = block_exclusive_scan<SCAN_T>(x, ComposeLq<Lq64>(), id, lds, &tot);
    if (t < T) local[t] = ex;
    if (threadIdx.x == 0) btot[blockIdx.x] = tot;
}

// info words
enum : int { FI_BASES = 0, FI_LINES_EFF = 1, FI_LINES = 2, FI_ERR = 3, FI_LEN_SEQ = 4, FI_LEN_QUAL = 5, FI_WORDS = 6 };

// Level 2 (one block): exclusive prefixes of the block totals, and the file
// totals (n_bases, the lines up to the last non-empty one, all lines).
__global__ __launch_bounds__(SCAN_T) void fq_scan_top(const Lq64 *__restrict__ btot, uint64_t NB,
                                                      Lq64 *__restrict__ bpre, uint64_t *__restrict__ info) {
    __shared__ Lq64 lds[SCAN_T / 64];
    const Lq64 id = lq_id<Lq64>();
    ComposeLq<Lq64> op;
    Lq64 carry = id;
    for (uint64_t b0 = 0; b0 < NB; b0 += SCAN_T) {
        const uint64_t b = b0 + threadIdx.x;
        const Lq64 x = b < NB ? btot[b] : id;
        Lq64 tot;
        const Lq64 ex = block_exclusive_scan<SCAN_T>(x, op, id, lds, &tot);
        if (b < NB) bpre[b] = op(carry, ex);
        carry = op(carry, tot);
    }
    if (threadIdx.x == 0) {
        info[FI_BASES] = carry.k[2];  // sequence lines: inclusive line count == 2 mod 4
        info[FI_LINES_EFF] = carry.last_ne;
        info[FI_LINES] = carry.lines;
        info[FI_ERR] = ~0ull;
        info[FI_LEN_SEQ] = info[FI_LEN_QUAL] = 0;
    }
}

__global__ __launch_bounds__(PT) void fq_emit(const uint8_t *__restrict__ text, uint64_t n,
                                              const Lq64 *__restrict__ local, const Lq64 *__restrict__ bpre,
                                              uint64_t n_eff, uint8_t *__restrict__ codes,
                                              uint64_t *__restrict__ rec_hdr, uint64_t *__restrict__ rec_seq,
                                              uint64_t *__restrict__ lstart) {
    __shared__ Lq lds[PT / 64];
    __shared__ __attribute__((aligned(16))) uint8_t stage[PTILE + 32];
    const uint32_t tb = blockIdx.x;
    const uint64_t pos = (uint64_t)tb * PTILE + (uint64_t)threadIdx.x * PB;
    Chunk ch;
    load_chunk(text, n, pos, ch);
    uint64_t em;         // this chunk's bytes of sequence lines
    uint32_t lk0, tile_kept;
    uint64_t tile_base;  // codes before this tile
    {
        uint64_t km[4];
        residue_masks(ch, km);
        const Lq x = chunk_lq(ch, km);
        Lq tot;
        const Lq pre = block_exclusive_scan<PT>(x, ComposeLq<Lq>(), lq_id<Lq>(), lds, &tot);
        const Lq64 p = ComposeLq<Lq64>()(bpre[tb / SCAN_T], local[tb]);
        tile_base = p.k[2];
        // a sequence byte has (lines before the tile + tile-local count) == 2 mod 4
        const uint32_t rt = (2u - (uint32_t)p.lines) & 3u;
        lk0 = sel4(pre.k, rt);
        tile_kept = sel4(tot.k, rt);
        em = sel4(km, (rt - pre.lines) & 3u);
        // line starts of this chunk: offsets of lines 0 .. n_eff (the end of the
        // last kept line), and the records opened by lines 0 mod 4
        uint64_t g = p.lines + pre.lines;
        for (uint64_t m = ch.ls; m; m &= m - 1, g++) {
            const int h = __ffsll((unsigned long long)m) - 1;
            if (g > n_eff) break;
            lstart[g] = pos + h;
            if ((g & 3u) == 0 && g < n_eff) {
                rec_hdr[g >> 2] = pos + h;
                rec_seq[g >> 2] = tile_base + lk0 + __popcll(em & bits_below(h));
            }
        }
    }
    // codes staged at the tile's output alignment, so LDS and HBM agree mod 16
    const uint32_t al = (uint32_t)(tile_base & 15u);
    const uint32_t lk = al + lk0;
    if (em) {
        uint32_t cw[PB / 4];
#pragma unroll
        for (int v = 0; v < PB / 4; v++) cw[v] = codes4(ch.w[v]);
        const int a = __ffsll((unsigned long long)em) - 1;
        const uint64_t run = em >> a;
        if ((run & (run + 1)) == 0) {
            // one run of bytes [a, a + cnt) (a sequence line crossing the chunk):
            // moved down to byte (lk & 3) in registers -- a word-granular barrel
            // shift, then one byte alignment -- and written as whole LDS words,
            // bytewise only where a word is shared with the neighbouring chunks.
            // Byte stores of lanes 64 bytes apart would all hit a few banks.
            const uint32_t wq = (uint32_t)a >> 2;
#pragma unroll
            for (int st = 8; st >= 1; st >>= 1) {
                const bool on = wq & st;
#pragma unroll
                for (int i = 0; i < PB / 4; i++) {
                    const uint32_t up = i + st < PB / 4 ? cw[i + st] : 0u;
                    cw[i] = on ? up : cw[i];
                }
            }
            const uint32_t sa = lk & 3u, a0 = lk >> 2;
            const int delta = (a & 3) - (int)sa;
            const uint32_t sel = (uint32_t)delta & 3u;
            const uint32_t e = lk + (uint32_t)__popcll(em);
            uint32_t *st32 = reinterpret_cast<uint32_t *>(stage);
            // wa(j) = bytes [4j + sel, 4j + sel + 4) of the word stream
            uint32_t prevw = __builtin_amdgcn_alignbyte(cw[0], 0u, sel);  // wa(-1)
#pragma unroll
            for (int j = 0; j <= PB / 4; j++) {
                const uint32_t lo = j < PB / 4 ? cw[j] : 0u, hi = j + 1 < PB / 4 ? cw[j + 1] : 0u;
                const uint32_t cur = __builtin_amdgcn_alignbyte(hi, lo, sel);
                const uint32_t word = delta < 0 ? prevw : cur;
                prevw = cur;
                const uint32_t wb = 4 * (a0 + (uint32_t)j);
                const uint32_t b0 = wb > lk ? wb : lk, b1 = wb + 4 < e ? wb + 4 : e;
                if (b0 >= b1) continue;
                if (b0 == wb && b1 == wb + 4) {
                    st32[a0 + j] = word;
                } else {
                    for (uint32_t b = b0; b < b1; b++) stage[b] = (uint8_t)(word >> (8 * (b - wb)));
                }
            }
        } else {
            // several short sequence lines in one chunk
            uint32_t o = lk;
#pragma unroll
            for (int i = 0; i < PB; i++) {
                if ((em >> i) & 1ull) stage[o++] = (uint8_t)byte_at(cw, i);
            }
        }
    }
    __syncthreads();
    // [al, al + tile_kept) of stage -> codes + tile_base: whole 16-byte words as
    // vectors, the two partial end words (shared with the neighbour tiles) bytewise
    uint8_t *dst = codes + (tile_base - al);
    const uint32_t end = al + tile_kept;
    const uint32_t nwords = (end + 15) / 16;
    for (uint32_t q = threadIdx.x; q < nwords; q += PT) {
        const uint32_t b0 = q * 16;
        if (b0 >= al && b0 + 16 <= end) {
            *reinterpret_cast<uint4 *>(dst + b0) = *reinterpret_cast<const uint4 *>(stage + b0);
        } else {
            for (uint32_t b = b0; b < b0 + 16; b++)
                if (b >= al && b < end) dst[b] = stage[b];
        }
    }
}

// bit 3 on the first code of every non-empty record
__global__ void fq_mark_records(uint8_t *__restrict__ codes, const uint64_t *__restrict__ rec_seq, uint64_t R,
                                uint64_t n_bases) {
    const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r < R) {
        const uint64_t p = rec_seq[r];
        if (p < n_bases && (r + 1 == R || rec_seq[r + 1] != p)) codes[p] |= 8;
    }
}

// Lengths (bytes before the terminator) and first bytes (0: empty) of record
// r's four lines, from the line start offsets; lines from n_eff on are padding.
// Returns the first rule the record breaks (1 '@', 2 '+', 3 lengths) or 0.
KMAN_DEV uint32_t fq_check_record(const uint8_t *text, uint64_t n, const uint64_t *lstart, uint64_t n_eff,
                                  uint64_t n_lines, uint64_t r, uint64_t &len_seq, uint64_t &len_qual) {
    uint64_t len[4];
    uint32_t first[4];
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const uint64_t g = 4 * r + i;
        len[i] = 0;
        first[i] = 0;
        if (g < n_eff) {
            const uint64_t s = lstart[g];
            const uint64_t e = g + 1 < n_lines ? lstart[g + 1] : n;
            uint64_t L = e - s;
            if (L) {
                const uint32_t c = text[e - 1];
                if (c == '\n') {
                    L--;
                    if (L && text[e - 2] == '\r') L--;
                } else if (c == '\r') {
                    L--;
                }
            }
            len[i] = L;
            first[i] = L ? text[s] : 0u;
        }
    }
    len_seq = len[1];
    len_qual = len[3];
    return first[0] != '@' ? 1u : (first[2] != '+' ? 2u : (len[3] != len[1] ? 3u : 0u));
}

__global__ void fq_validate(const uint8_t *__restrict__ text, uint64_t n, const uint64_t *__restrict__ lstart,
                            uint64_t n_eff, uint64_t n_lines, uint64_t R, uint64_t *__restrict__ info) {
    const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= R) return;
    uint64_t ls, lq;
    const uint32_t rule = fq_check_record(text, n, lstart, n_eff, n_lines, r, ls, lq);
    if (rule) atomicMin((unsigned long long *)&info[FI_ERR], (unsigned long long)((r << 2) | rule));
}

// the first offending record's two lengths, for the message
__global__ void fq_report(const uint8_t *__restrict__ text, uint64_t n, const uint64_t *__restrict__ lstart,
                          uint64_t n_eff, uint64_t n_lines, uint64_t *__restrict__ info) {
    const uint64_t err = info[FI_ERR];
    if (err == ~0ull) return;
    uint64_t ls, lq;
    (void)fq_check_record(text, n, lstart, n_eff, n_lines, err >> 2, ls, lq);
    info[FI_LEN_SEQ] = ls;
    info[FI_LEN_QUAL] = lq;
}


// ---------------------------------------------------------------- quality mask
// bits of the tile's codes [0, al + tile_kept), al <= 15, in 32-bit words
constexpr int QBM_WORDS = (PTILE + 16 + 31) / 32 + 3;

// the four text bytes at `off` (off % 4 == 0; the text is 16-byte aligned),
// zeros past the end of the text
KMAN_DEV uint32_t text_word(const uint8_t *text, uint64_t n, uint64_t off) {
    if (off + 4 <= n) return *reinterpret_cast<const uint32_t *>(text + off);
    uint32_t v = 0;
#pragma unroll
    for (int b = 0; b < 4; b++) v |= (off + b < n ? (uint32_t)text[off + b] : 0u) << (8 * b);
    return v;
}
// codes of four bases, those picked by the 4-bit mask x turned into an N's
// (4, bit 3 kept)
KMAN_DEV uint32_t mask_codes4(uint32_t c, uint32_t x) {
    const uint32_t mm = ((x * 0x00204081u) & 0x01010101u) * 0xffu;
    return (c & ~mm) | (((c & 0x08080808u) | 0x04040404u) & mm);
}

// The codes of the kept sequence bytes whose quality byte is below T become
// 4 | (code & 8).  fq_emit's geometry and prefixes give every chunk its
// sequence-byte mask, the index of its first code and the line of each run of
// sequence bytes; the quality bytes of a run sit lstart[g + 2] - lstart[g]
// further on.  The low-quality bits of a chunk, compacted to its codes, are
// OR-ed into a bit map of the tile's codes in LDS (2 KiB; three LDS atomics
// per chunk at most); then the tile's codes are rewritten as 16-byte vectors
// at their own alignment, skipping the vectors without a masked code, the two
// end vectors shared with the neighbour tiles bytewise.  Runs after
// fq_validate has passed, so line g + 2 exists and is as long as line g.
__global__ __launch_bounds__(PT) void fq_qmask(const uint8_t *__restrict__ text, uint64_t n,
                                               const Lq64 *__restrict__ local, const Lq64 *__restrict__ bpre,
                                               const uint64_t *__restrict__ lstart, uint64_t n_eff, uint32_t T,
                                               uint8_t *__restrict__ codes,
                                               unsigned long long *__restrict__ n_masked) {
    __shared__ Lq lds[PT / 64];
    __shared__ uint32_t cnt_lds[PT / 64];
    __shared__ uint32_t bm[QBM_WORDS];
    for (uint32_t i = threadIdx.x; i < (uint32_t)QBM_WORDS; i += PT) bm[i] = 0;  // (the scan's barriers order this)
    const uint32_t tb = blockIdx.x;
    const uint64_t pos = (uint64_t)tb * PTILE + (uint64_t)threadIdx.x * PB;
    Chunk ch;
    load_chunk(text, n, pos, ch);
    uint64_t em;   // this chunk's bytes of sequence lines
    uint64_t L0;   // lines started before this chunk
    uint32_t lk0, tile_kept;
    uint64_t tile_base;
    {
        uint64_t km[4];
        residue_masks(ch, km);
        const Lq x = chunk_lq(ch, km);
        Lq tot;
        const Lq pre = block_exclusive_scan<PT>(x, ComposeLq<Lq>(), lq_id<Lq>(), lds, &tot);
        const Lq64 p = ComposeLq<Lq64>()(bpre[tb / SCAN_T], local[tb]);
        tile_base = p.k[2];
        const uint32_t rt = (2u - (uint32_t)p.lines) & 3u;
        lk0 = sel4(pre.k, rt);
        tile_kept = sel4(tot.k, rt);
        em = sel4(km, (rt - pre.lines) & 3u);
        L0 = p.lines + pre.lines;
    }
    const uint32_t al = (uint32_t)(tile_base & 15u);
    uint32_t nm = 0;
    if (em) {
        uint64_t mc = 0;  // bit o: the chunk's o-th code is masked
        const int a = __ffsll((unsigned long long)em) - 1;
        const uint64_t run = em >> a;
        if ((run & (run + 1)) == 0) {
            // one run [a, a + cnt): its line is the one byte a lies in
            const uint64_t g = L0 + (uint64_t)__popcll(ch.ls & bits_below(a + 1)) - 1;
            if (g + 2 <= n_eff) {
                // the 64 bytes at pos + delta, unaligned: 17 dwords, byte-aligned in pairs
                const uint64_t qpos = pos + (lstart[g + 2] - lstart[g]);
                const uint64_t off0 = qpos & ~3ull;
                const uint32_t sh = (uint32_t)(qpos & 3u);
                uint32_t d[PB / 4 + 1];
#pragma unroll
                for (int j = 0; j <= PB / 4; j++) d[j] = text_word(text, n, off0 + 4 * (uint64_t)j);
                uint64_t low = 0;
#pragma unroll
                for (int v = 0; v < PB / 4; v++) {
                    const uint32_t qw = __builtin_amdgcn_alignbyte(d[v + 1], d[v], sh);
                    low |= (uint64_t)hibits4(lt_bytes_u8(qw, T)) << (4 * v);
                }
                mc = (em & low) >> a;
            }
        } else {
            // several runs in one chunk (short lines, or blanks inside a line)
            uint32_t o = 0;
            for (uint64_t m = em; m; m &= m - 1, o++) {
                const int i = __ffsll((unsigned long long)m) - 1;
                const uint64_t g = L0 + (uint64_t)__popcll(ch.ls & bits_below(i + 1)) - 1;
                if (g + 2 > n_eff) continue;
                const uint64_t qp = pos + (uint64_t)i + (lstart[g + 2] - lstart[g]);
                if (qp < n && (uint32_t)text[qp] < T) mc |= 1ull << o;
            }
        }
        nm = (uint32_t)__popcll(mc);
        if (mc) {
            const uint32_t lk = al + lk0, w0 = lk >> 5, s = lk & 31u;
            const uint64_t lo = mc << s;
            const uint32_t x0 = (uint32_t)lo, x1 = (uint32_t)(lo >> 32), x2 = s ? (uint32_t)(mc >> (64 - s)) : 0u;
            if (x0) atomicOr(&bm[w0], x0);
            if (x1) atomicOr(&bm[w0 + 1], x1);
            if (x2) atomicOr(&bm[w0 + 2], x2);
        }
    }
    uint32_t nm_tile;
    (void)block_exclusive_scan<PT>(nm, SumU32(), 0u, cnt_lds, &nm_tile);  // (its barriers publish bm)
    if (nm_tile == 0) return;
    if (threadIdx.x == 0) atomicAdd(n_masked, (unsigned long long)nm_tile);
    uint8_t *dst = codes + (tile_base - al);
    const uint32_t end = al + tile_kept;
    const uint32_t nwords = (end + 15) / 16;
    for (uint32_t q = threadIdx.x; q < nwords; q += PT) {
        const uint32_t bits = (bm[q >> 1] >> (16 * (q & 1u))) & 0xffffu;
        if (!bits) continue;
        const uint32_t b0 = q * 16;
        if (b0 >= al && b0 + 16 <= end) {
            uint4 c = *reinterpret_cast<const uint4 *>(dst + b0);
            c.x = mask_codes4(c.x, bits & 15u);
            c.y = mask_codes4(c.y, (bits >> 4) & 15u);
            c.z = mask_codes4(c.z, (bits >> 8) & 15u);
            c.w = mask_codes4(c.w, bits >> 12);
            *reinterpret_cast<uint4 *>(dst + b0) = c;
        } else {
            for (uint32_t b = 0; b < 16; b++)  // (bits are set inside [al, end) only)
                if ((bits >> b) & 1u) dst[b0 + b] = (uint8_t)(4u | (dst[b0 + b] & 8u));
        }
    }
}

// qbyte: the quality threshold byte (0: no mask pass); n_masked may be null
int parse_fastq(kman_ctx *ctx, const uint8_t *d_text, uint64_t n_bytes, uint8_t *d_codes, uint64_t *d_rec_hdr,
                uint64_t *d_rec_seq, uint64_t rec_cap, kman_parse_info *info, uint32_t qbyte, uint64_t *n_masked) {
    if (!ctx || !info) return KMAN_EINVAL;
    info->n_bases = info->n_records = 0;
    if (n_masked) *n_masked = 0;
    if (qbyte > 255) return kman_fail(ctx, KMAN_EINVAL, "quality threshold byte %u > 255", qbyte);
    if (n_bytes && (!d_text || !d_codes)) return kman_fail(ctx, KMAN_EINVAL, "null buffer");
    if (((uintptr_t)d_text & 15) != 0) return kman_fail(ctx, KMAN_EINVAL, "text must be 16-byte aligned");
    if (((uintptr_t)d_codes & 15) != 0) return kman_fail(ctx, KMAN_EINVAL, "codes must be 16-byte aligned");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const uint64_t T = n_bytes ? ceil_div(n_bytes, PTILE) : 0;
    if (T == 0) return kman_fail(ctx, KMAN_EFORMAT, "premature end of file or empty file");
    // scratch: tile summaries, their in-block prefixes, block totals and
    // prefixes (Lq64 each), info
    const uint64_t NB = ceil_div(T, (uint64_t)SCAN_T);
    const size_t q_bytes = ((T * sizeof(Lq64)) + 255) & ~size_t(255);
    const size_t nb_bytes = ((NB * sizeof(Lq64)) + 255) & ~size_t(255);
    void *scr;
    KMAN_TRY(kman_scratch(ctx, 2 * q_bytes + 2 * nb_bytes + 256, &scr));
    Lq64 *d_q = (Lq64 *)scr;
    Lq64 *d_local = (Lq64 *)((char *)scr + q_bytes);
    Lq64 *d_btot = (Lq64 *)((char *)scr + 2 * q_bytes);
    Lq64 *d_bpre = (Lq64 *)((char *)scr + 2 * q_bytes + nb_bytes);
    uint64_t *d_info = (uint64_t *)((char *)scr + 2 * q_bytes + 2 * nb_bytes);
    { KTimer kt_(ctx, "parse_fastq");
    hipLaunchKernelGGL(fq_reduce, dim3((uint32_t)T), dim3(PT), 0, ctx->stream, d_text, n_bytes, d_q);
    hipLaunchKernelGGL(fq_scan_blocks, dim3((uint32_t)NB), dim3(SCAN_T), 0, ctx->stream, d_q, T, d_local, d_btot);
    hipLaunchKernelGGL(fq_scan_top, dim3(1), dim3(SCAN_T), 0, ctx->stream, d_btot, NB, d_bpre, d_info); }
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipMemcpyAsync(ctx->h_small, d_info, 3 * sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    const uint64_t n_bases = ctx->h_small[FI_BASES], n_eff = ctx->h_small[FI_LINES_EFF],
                   n_lines = ctx->h_small[FI_LINES];
    if (n_eff == 0) return kman_fail(ctx, KMAN_EFORMAT, "premature end of file or empty file");
    const uint64_t R = ceil_div(n_eff, 4);
    if (R > rec_cap)
        return kman_fail(ctx, KMAN_ECAP, "record capacity %llu < %llu", (unsigned long long)rec_cap,
                         (unsigned long long)R);
    if (!d_rec_hdr || !d_rec_seq) return kman_fail(ctx, KMAN_EINVAL, "null buffer");
    // line start offsets of lines 0 .. n_eff
    void *aux;
    KMAN_TRY(kman_aux(ctx, (n_eff + 1) * sizeof(uint64_t), &aux));
    uint64_t *d_lstart = (uint64_t *)aux;
    { KTimer kt_(ctx, "parse_fastq");
    hipLaunchKernelGGL(fq_emit, dim3((uint32_t)T), dim3(PT), 0, ctx->stream, d_text, n_bytes, d_local, d_bpre, n_eff,
                       d_codes, d_rec_hdr, d_rec_seq, d_lstart);
    hipLaunchKernelGGL(fq_mark_records, dim3((uint32_t)ceil_div(R, 256)), dim3(256), 0, ctx->stream, d_codes,
                       d_rec_seq, R, n_bases);
    hipLaunchKernelGGL(fq_validate, dim3((uint32_t)ceil_div(R, 256)), dim3(256), 0, ctx->stream, d_text, n_bytes,
                       d_lstart, n_eff, n_lines, R, d_info);
    hipLaunchKernelGGL(fq_report, dim3(1), dim3(1), 0, ctx->stream, d_text, n_bytes, d_lstart, n_eff, n_lines,
                       d_info); }
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipMemsetAsync(d_codes + n_bases, 4, 64, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(ctx->h_small, d_info, FI_WORDS * sizeof(uint64_t), hipMemcpyDeviceToHost,
                                ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    const uint64_t err = ctx->h_small[FI_ERR];
    if (err != ~0ull) {
        const unsigned long long rec = (unsigned long long)(err >> 2) + 1;
        switch (err & 3u) {
        case 1: return kman_fail(ctx, KMAN_EFORMAT, "FASTQ record %llu: header line does not start with '@'", rec);
        case 2: return kman_fail(ctx, KMAN_EFORMAT, "FASTQ record %llu: separator line does not start with '+'", rec);
        default:
            return kman_fail(ctx, KMAN_EFORMAT, "FASTQ record %llu: quality length %llu != sequence length %llu", rec,
                             (unsigned long long)ctx->h_small[FI_LEN_QUAL],
                             (unsigned long long)ctx->h_small[FI_LEN_SEQ]);
        }
    }
    if (qbyte) {
        // the tile prefixes are still in the scratch, the line starts in aux
        unsigned long long *d_nm = (unsigned long long *)(d_info + FI_WORDS + 2);
        HIP_TRY(ctx, hipMemsetAsync(d_nm, 0, sizeof(*d_nm), ctx->stream));
        { KTimer kt_(ctx, "parse_fastq");
        hipLaunchKernelGGL(fq_qmask, dim3((uint32_t)T), dim3(PT), 0, ctx->stream, d_text, n_bytes, d_local, d_bpre,
                           d_lstart, n_eff, qbyte, d_codes, d_nm); }
        HIP_TRY(ctx, hipGetLastError());
        HIP_TRY(ctx, hipMemcpyAsync(ctx->h_small, d_nm, sizeof(*d_nm), hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        if (n_masked) *n_masked = ctx->h_small[0];
    }
    info->n_bases = n_bases;
    info->n_records = R;
    return KMAN_OK;
}

}  // namespace

extern "C" int kman_parse_fastq(kman_ctx *ctx, const uint8_t *d_text, uint64_t n_bytes, uint8_t *d_codes,
                                uint64_t *d_rec_hdr, uint64_t *d_rec_seq, uint64_t rec_cap,
                                kman_parse_info *info) {
    return parse_fastq(ctx, d_text, n_bytes, d_codes, d_rec_hdr, d_rec_seq, rec_cap, info, 0, nullptr);
}

extern "C" int kman_parse_fastq_q(kman_ctx *ctx, const uint8_t *d_text, uint64_t n_bytes, uint8_t *d_codes,
                                  uint64_t *d_rec_hdr, uint64_t *d_rec_seq, uint64_t rec_cap,
                                  kman_parse_info *info, uint32_t min_qual_byte, uint64_t *n_masked) {
    return parse_fastq(ctx, d_text, n_bytes, d_codes, d_rec_hdr, d_rec_seq, rec_cap, info, min_qual_byte, n_masked);
}
