// correct.hip — isolated substitution errors of reads, repaired against a
// k-mer count table (`kmer screen --solid C --correct`).  Over
// kman_window_counts' words, a window start is WEAK when its word is not
// KMAN_WC_NONE and < min_count, SOLID when it is not KMAN_WC_NONE and >=
// min_count.  A weak run [a, b) of a record with bases [s, e) is a maximal
// interval of weak window starts inside [s, e).  With
//     L = a > s and a - 1 solid        openL = a == s
//     R = b + k <= e and b solid       openR = b + k == e + 1
// the run names the site p = b - 1 when (L and R and b - a == k) or (openL and
// R and b - a <= k), p = a + k - 1 when (L and openR and b - a <= k), and no
// site otherwise.  The windows of the record that cover p are then exactly the
// run's.  With o the base at p, the site is corrected to x != o when x is the
// only one of the three for which every window of the run, with x at p, has a
// count >= min_count in the table (the canonical key under KMAN_CANONICAL).
//
//   sites   kman_correct_sites, one block of 256 threads per tile of CTILE =
//           4096 bases.  The tile's words and a halo of CHALO >= 33 go to LDS,
//           with the word before the tile; thread 0 cuts the tile's slice of
//           d_rec_seq (tile_records.h: staged when <= CCAP entries, searched in
//           global memory above).  A wave owns 1024 consecutive bases, 64 at a
//           time, one per lane.  A lane whose base is weak finds its record
//           (one search); it is a run's START when the base is the record's
//           first or the base before it is not weak.  A start reads at most k
//           more words to find b (a longer run names no site), so nothing is
//           carried across tiles, and decides the case.  The wave then takes
//           its lanes' sites one after the other (a ballot, lowest lane
//           first): the lanes load the 64 codes from a on and two ballots
//           turn them into two 64-bit planes, from which a lane cuts its
//           window, puts x at p and interleaves the key (and its reverse
//           complement) without a loop.  Item i < 3 (b - a) <= 96 is
//           candidate i / (b - a) in window i % (b - a): lane l takes items l
//           and l + 64, one table_lookup<1, CT> each (screen_lookup.h).
//           ok(x) is a ballot.  The site's lane 0 stores d_fix[p]: every byte
//           of d_fix has one writer after the call's own 0xFF fill.  The
//           count of corrected bases is one atomic add per wave that has any.
//   codes   kman_apply_fixes: one thread per 16 bases, codes[b] = fix[b] |
//           (codes[b] & 8) where fix[b] != 0xFF.
//   text    kman_apply_fixes: one wave per record.  It counts the record's
//           fixes (64 lanes x 16 B of d_fix per step) and stores d_nfix[r].
//           With a text and at least one fix it finds line 2 as cut.hip's
//           trimming wave does (the record's first two terminator starts),
//           then walks it once, 1024 bytes per step: a lane's bytes that are
//           not ' ' are the kept characters, their code indices come from a
//           popcount, a DPP wave scan and a running total, and a kept
//           character whose base has a fix is stored as one byte.  A record of
//           L bytes takes about L / 1024 steps of one wave; there is no
//           block-per-record path for very long reads (cut.hip's limit).
//
// Bounds, not values: tile_records.h for the slice; a record's bounds are
// clamped (s <= a < e <= n_bases) before they are used; a start reads LDS
// words at most k past its own (< CTILE + CHALO); p < e, so d_fix is written
// below n_bases; codes are read below n_bases + 64 (the parsers' padding); the
// table is read through table_lookup's clamps.  A text byte is read and
// written only inside its record's clamped byte range, a fix only below the
// record's end.  A d_wc, index, d_rec_seq or d_fix that does not belong to
// these codes gives wrong corrections, never a wild address or an unbounded
// loop.
//
// Algorithmic bytes of kman_correct_sites: 4 B read per base (the words, plus
// the halo), 1 B written per base (the fill); per site 64 B of codes, at most
// 3 k lookups (screen.hip's bytes per lookup) and one byte stored.
#include "common.h"
#include "bytes16.h"
#include "screen_lookup.h"
#include "tile_records.h"

namespace {

constexpr int CT_ = 256;
constexpr int CTILE = KMAN_CORRECT_TILE;
constexpr int CHALO = 36;  // words staged past the tile: a start reads at most k = 32 past its own
constexpr int CCAP = KMAN_CORRECT_REC_CAP;
constexpr int CPW = CTILE / (CT_ / 64);  // bases per wave
constexpr uint32_t NOFIX = KMAN_FIX_NONE;
static_assert(CHALO >= 33 && CHALO % 4 == 0, "k + 1 words past a start, staged in 16-byte vectors");
static_assert(CPW % 64 == 0, "a wave walks its bases 64 at a time");

#define WC_NONE KMAN_WC_NONE

KMAN_DEV bool is_weak(uint32_t w, uint32_t c) { return w != WC_NONE && w < c; }
KMAN_DEV bool is_solid(uint32_t w, uint32_t c) { return w != WC_NONE && w >= c; }

// bit i of the low 32 bits of x to bit 2 i
KMAN_DEV uint64_t spread2(uint64_t x) {
    x &= 0xffffffffull;
    x = (x | (x << 16)) & 0x0000ffff0000ffffull;
    x = (x | (x << 8)) & 0x00ff00ff00ff00ffull;
    x = (x | (x << 4)) & 0x0f0f0f0f0f0f0f0full;
    x = (x | (x << 2)) & 0x3333333333333333ull;
    x = (x | (x << 1)) & 0x5555555555555555ull;
    return x;
}

// The key of the window of k bases whose low / high code bits are bits
// 0 .. k - 1 of m0 / m1 (bit 0: the first base): the first base most
// significant; CANON: the smaller of it and its reverse complement.
template <int CANON>
KMAN_DEV uint64_t key_of_planes(uint64_t m0, uint64_t m1, int k, uint64_t mask) {
    // reversed, the first base sits in the top pair of the 2k bits
    const uint64_t r0 = __brevll(m0) >> (64 - k), r1 = __brevll(m1) >> (64 - k);
    const uint64_t fwd = spread2(r0) | (spread2(r1) << 1);
    if (!CANON) return fwd;
    // unreversed, the last base sits there: the reverse, complemented
    const uint64_t rc = (spread2(m0) | (spread2(m1) << 1)) ^ mask;
    return fwd < rc ? fwd : rc;
}

template <int CANON, typename CT>
__global__ __launch_bounds__(CT_) void correct_sites_kernel(
    const uint8_t *__restrict__ codes, uint64_t n_bases, int k, const uint32_t *__restrict__ wc,
    const uint64_t *__restrict__ rec_seq, uint64_t n_records, const uint64_t *__restrict__ tkeys,
    const CT *__restrict__ tcounts, uint64_t nt, const uint64_t *__restrict__ index, uint32_t shift,
    uint32_t min_count, uint8_t *__restrict__ fix, unsigned long long *__restrict__ n_fixed) {
    __shared__ __attribute__((aligned(16))) uint32_t sw[CTILE + CHALO];
    __shared__ uint64_t srec[CCAP + 1];
    __shared__ uint64_t s_r0, s_ns, s_next;
    __shared__ uint32_t s_prev;

    const uint64_t tb = (uint64_t)blockIdx.x * CTILE;
    const uint64_t tend = umin64(tb + CTILE, n_bases);  // (tb < n_bases: the grid is ceil(n_bases / CTILE))
    if (threadIdx.x == 0) {
        const TileSlice s = cut_slice(rec_seq, n_records, tb, tend - 1, n_bases);  // the records that own [tb, tend)
        s_r0 = s.r0;
        s_ns = s.ns;
        s_next = s.next;
        s_prev = tb ? wc[tb - 1] : WC_NONE;
    }
    // the tile's words and the halo (past n_bases: NONE, neither weak nor solid)
    for (uint32_t i = threadIdx.x; i < (uint32_t)((CTILE + CHALO) / 4); i += CT_) {
        const uint64_t b = tb + 4ull * i;
        uint4 v = make_uint4(WC_NONE, WC_NONE, WC_NONE, WC_NONE);
        if (b + 4 <= n_bases) {
            v = *reinterpret_cast<const uint4 *>(wc + b);
        } else {
            if (b < n_bases) v.x = wc[b];
            if (b + 1 < n_bases) v.y = wc[b + 1];
            if (b + 2 < n_bases) v.z = wc[b + 2];
        }
        *reinterpret_cast<uint4 *>(sw + 4 * i) = v;
    }
    __syncthreads();
    const uint64_t r0 = s_r0, ns = s_ns, next = s_next;
    if (ns == 0) return;  // (no record starts at or before the tile's last base; block-uniform)
    const SliceView sv = stage_slice<CT_, CCAP>(rec_seq, {r0, ns, next}, srec);
    if (!sv.big) __syncthreads();  // (block-uniform)
    const uint64_t *rs = sv.rs;

    const int lane = lane_id();
    const uint32_t wbase = (threadIdx.x >> 6) * (uint32_t)CPW;
    const uint64_t mask = k == 32 ? ~0ull : ((1ull << (2 * k)) - 1);
    const uint64_t km = k == 32 ? 0xffffffffull : ((1ull << k) - 1);
    uint32_t fixed = 0;  // (wave-uniform)

    for (uint32_t it = 0; it < (uint32_t)CPW; it += 64) {
        const uint32_t i = wbase + it + (uint32_t)lane;  // < CTILE
        const uint64_t a = tb + i;
        if (tb + wbase + it >= n_bases) break;  // (wave-uniform)
        const uint32_t w = sw[i];
        // a site of this lane: its run [a, a + len), the base p
        uint32_t len = 0;
        uint64_t p = 0;
        if (a < n_bases && is_weak(w, min_count)) {
            const uint64_t u = upper_count(rs, ns, a);
            if (u != 0) {  // (0: a base before the first record)
                const uint64_t s = umin64(rs[u - 1], a);
                const uint64_t e = umin64(sv.ent(u), n_bases);
                const uint32_t before = i ? sw[i - 1] : s_prev;
                if (e > a && (a == s || !is_weak(before, min_count))) {
                    // b: the first window start after a that is not weak, or e; given up past a + k
                    uint32_t j = 1;
                    while (j <= (uint32_t)k && a + j < e && is_weak(sw[i + j], min_count)) j++;
                    if (j <= (uint32_t)k) {
                        const uint64_t b = a + j;
                        const bool L = a > s && is_solid(before, min_count);
                        const bool R = b + (uint64_t)k <= e && is_solid(sw[i + j], min_count);
                        const bool openL = a == s, openR = b + (uint64_t)k == e + 1;
                        if (R && ((L && j == (uint32_t)k) || openL)) {
                            len = j;
                            p = b - 1;
                        } else if (L && openR) {
                            len = j;
                            p = a + (uint64_t)k - 1;
                        }
                    }
                }
            }
        }
        // the wave's sites of this round, lowest lane first
        uint64_t todo = __ballot(len != 0);
        while (todo) {  // (wave-uniform)
            const int src = __ffsll((unsigned long long)todo) - 1;
            todo &= todo - 1;
            const uint32_t slen = (uint32_t)__shfl((int)len, src, 64);   // 1 .. k
            const uint64_t sa = tb + wbase + it + (uint32_t)src;           // the run's first window
            const uint32_t q = (uint32_t)(shfl_any(p, src) - sa);         // p - sa: slen - 1 or k - 1, < 32
            // codes sa .. sa + 63 as two planes (sa < n_bases, 64 bytes of padding follow the codes)
            const uint32_t c = codes[sa + (uint32_t)lane];
            const uint64_t P0 = __ballot((c & 1u) != 0), P1 = __ballot((c & 2u) != 0);
            const uint32_t o = (uint32_t)((P0 >> q) & 1u) | ((uint32_t)((P1 >> q) & 1u) << 1);
            uint32_t fail = 0;  // bit c: candidate c has a window below min_count
#pragma unroll
            for (int t = 0; t < 2; t++) {
                const uint32_t item = (uint32_t)lane + 64u * t;
                const bool on = item < 3 * slen;
                const uint32_t cand = on ? item / slen : 0u, win = on ? item - cand * slen : 0u;
                const uint32_t x = (o + 1 + cand) & 3u;
                const uint32_t at = q - win;  // p inside the window: 0 .. k - 1
                uint64_t m0 = (P0 >> win) & km, m1 = (P1 >> win) & km;
                m0 = (m0 & ~(1ull << at)) | ((uint64_t)(x & 1u) << at);
                m1 = (m1 & ~(1ull << at)) | ((uint64_t)(x >> 1) << at);
                uint64_t kf[1] = {key_of_planes<CANON>(m0, m1, k, mask)}, cnt[1];
                table_lookup<1, CT>(on ? 1u : 0u, kf, shift, index, tkeys, tcounts, nt, cnt);
                const bool bad = on && cnt[0] < (uint64_t)min_count;
#pragma unroll
                for (uint32_t cc = 0; cc < 3; cc++)
                    if (__ballot(bad && cand == cc)) fail |= 1u << cc;
            }
            const uint32_t okm = ~fail & 7u;
            if (okm && (okm & (okm - 1)) == 0) {  // exactly one candidate stands
                const uint32_t cand = (uint32_t)__ffs((int)okm) - 1u;
                if (lane == 0) fix[sa + q] = (uint8_t)((o + 1 + cand) & 3u);
                fixed++;
            }
        }
    }
    if (fixed && lane == 0) atomicAdd(n_fixed, (unsigned long long)fixed);
}

template <int CANON, typename CT>
void launch_correct_sites(kman_ctx *ctx, const uint8_t *codes, uint64_t n_bases, uint32_t k, const uint32_t *wc,
                          const uint64_t *rec_seq, uint64_t n_records, const uint64_t *tkeys, const void *tcounts,
                          uint64_t nt, const uint64_t *index, uint32_t shift, uint32_t min_count, uint8_t *fix,
                          unsigned long long *n_fixed, uint64_t tiles) {
    hipLaunchKernelGGL((correct_sites_kernel<CANON, CT>), dim3((uint32_t)tiles), dim3(CT_), 0, ctx->stream, codes,
                       n_bases, (int)k, wc, rec_seq, n_records, tkeys, (const CT *)tcounts, nt, index, shift, min_count,
                       fix, n_fixed);
}

// ------------------------------------------------------------ apply

// codes[b] = fix[b] | (codes[b] & 8) where fix[b] != 0xFF; 16 bases per thread
__global__ __launch_bounds__(CT_) void apply_codes_kernel(uint8_t *__restrict__ codes, uint64_t n_bases,
                                                          const uint8_t *__restrict__ fix) {
    const uint64_t b0 = 16ull * ((uint64_t)blockIdx.x * CT_ + threadIdx.x);
    if (b0 >= n_bases) return;
    if (b0 + 16 <= n_bases) {
        const uint4 f = *reinterpret_cast<const uint4 *>(fix + b0);
        if ((f.x & f.y & f.z & f.w) == 0xFFFFFFFFu) return;  // (nearly every vector)
    }
    for (int j = 0; j < 16; j++) {
        const uint64_t b = b0 + j;
        if (b >= n_bases) break;
        const uint32_t x = fix[b];
        if (x != NOFIX) codes[b] = (uint8_t)((x & 3u) | (codes[b] & 8u));
    }
}

// one wave per record: d_nfix[r], and the text bytes of its fixed bases
__global__ __launch_bounds__(CT_) void apply_records_kernel(const uint8_t *__restrict__ fix, uint64_t n_bases,
                                                            const uint64_t *__restrict__ rec_seq, uint64_t n_records,
                                                            uint8_t *text, uint64_t n_bytes,
                                                            const uint64_t *__restrict__ rec_off,
                                                            uint32_t *__restrict__ nfix) {
    const uint64_t r = (uint64_t)blockIdx.x * (CT_ / 64) + (threadIdx.x >> 6);
    if (r >= n_records) return;  // (the whole wave)
    const int lane = lane_id();
    const uint64_t s = umin64(rec_seq[r], n_bases);
    const uint64_t e = r + 1 < n_records ? umin64(rec_seq[r + 1], n_bases) : n_bases;  // (e <= s: an empty record)
    uint32_t total = 0;
    for (uint64_t base = s & ~15ull; base < e; base += 1024) {
        const uint64_t p = base + 16ull * (uint32_t)lane;
        uint32_t n = 0;
        if (p < e) {
            const uint4 f = load16<NOFIX>(fix, n_bases, p);
#pragma unroll
            for (int j = 0; j < 16; j++) n += (p + j >= s && p + j < e && byte_of(f, j) != NOFIX) ? 1u : 0u;
        }
        total += (uint32_t)__shfl((int)wave_inclusive_scan(n, SumU32(), 0u), 63, 64);
    }
    if (lane == 0) nfix[r] = total;
    if (!text || total == 0) return;  // (wave-uniform)

    const uint64_t a = umin64(rec_off[r], n_bytes), b = umin64(rec_off[r + 1], n_bytes);
    if (b <= a) return;
    // the record's first two terminator starts (b: the line runs to the record's end)
    uint64_t t0 = b, t1 = b;
    uint32_t found = 0;
    for (uint64_t base = a & ~15ull; base < b && found < 2; base += 1024) {
        const uint64_t p = base + 16ull * (uint32_t)lane;
        uint32_t m = 0;
        if (p < b) {
            const uint4 v = load16(text, n_bytes, p);
            uint32_t prev = p > a ? text[p - 1] : 0u;  // (the byte before the record never joins a "\r\n")
#pragma unroll
            for (int j = 0; j < 16; j++) {
                const uint32_t c = byte_of(v, j);
                const uint64_t pos = p + j;
                if (pos >= a && pos < b && (c == '\r' || (c == '\n' && prev != '\r'))) m |= 1u << j;
                prev = pos >= a ? c : 0u;
            }
        }
        uint64_t bal = __ballot(m != 0);
        while (bal && found < 2) {
            const int L = __ffsll((unsigned long long)bal) - 1;
            uint32_t lm = (uint32_t)__shfl((int)m, L, 64);
            while (lm && found < 2) {
                const uint64_t pos = base + 16ull * (uint32_t)L + ((uint32_t)__ffs((int)lm) - 1u);
                if (found == 0) t0 = pos;
                else t1 = pos;
                found++;
                lm &= lm - 1;
            }
            bal &= bal - 1;
        }
    }
    const uint64_t s2 = line_after(text, t0, b), e2 = t1;
    // line 2 once: the kept characters (not ' ') in order are the record's codes
    const uint64_t ncodes = e > s ? e - s : 0;
    uint64_t seen = 0;
    for (uint64_t base = s2 & ~15ull; base < e2 && seen < ncodes; base += 1024) {
        const uint64_t p = base + 16ull * (uint32_t)lane;
        uint32_t nb = 0;
        uint4 v = make_uint4(0, 0, 0, 0);
        if (p < e2) {
            v = load16(text, n_bytes, p);
#pragma unroll
            for (int j = 0; j < 16; j++)
                if (p + j >= s2 && p + j < e2 && byte_of(v, j) != ' ') nb |= 1u << j;
        }
        const uint32_t cnt = (uint32_t)__popc(nb);
        const uint32_t inc = wave_inclusive_scan(cnt, SumU32(), 0u);
        uint64_t ci = seen + (inc - cnt);  // the code index of the lane's first kept character
#pragma unroll
        for (int j = 0; j < 16; j++) {
            if (!((nb >> j) & 1u)) continue;
            if (ci < ncodes) {
                const uint32_t x = fix[s + ci];  // (s + ci < e <= n_bases)
                if (x != NOFIX) {
                    const uint32_t old = byte_of(v, j);
                    const uint32_t lower = old >= 'a' && old <= 'z' ? 0x20u : 0u;
                    // "ACGT" as the bytes of one word (p + j < e2 <= n_bytes)
                    text[p + j] = (uint8_t)(((0x54474341u >> (8 * (x & 3u))) & 0xffu) | lower);
                }
            }
            ci++;
        }
        seen += (uint32_t)__shfl((int)inc, 63, 64);
    }
}

}  // namespace

extern "C" int kman_correct_sites(kman_ctx *ctx, const uint8_t *d_codes, uint64_t n_bases, uint32_t k, uint32_t flags,
                                  const uint32_t *d_wc, const uint64_t *d_rec_seq, uint64_t n_records,
                                  const uint64_t *d_tkeys, const void *d_tcounts, uint32_t t_count_bytes, uint64_t nt,
                                  const uint64_t *d_index, uint32_t index_bits, uint32_t min_count, uint8_t *d_fix,
                                  uint64_t *n_fixed) {
    if (!ctx) return KMAN_EINVAL;
    if (n_fixed) *n_fixed = 0;
    if (k < 2 || k > 32) return kman_fail(ctx, KMAN_EINVAL, "k must be in [2, 32] on the GPU path, got %u", k);
    if (flags & ~KMAN_CANONICAL) return kman_fail(ctx, KMAN_EINVAL, "kman_correct_sites: flags 0x%x", flags);
    if (t_count_bytes != 4 && t_count_bytes != 8)
        return kman_fail(ctx, KMAN_EINVAL, "count widths must be 4 or 8 bytes");
    if (!index_bits_ok(k, index_bits))
        return kman_fail(ctx, KMAN_EINVAL, "index_bits must be in [1, min(2k, %d)], got %u (k = %u)",
                         KMAN_SCREEN_MAX_INDEX_BITS, index_bits, k);
    if (min_count < 1 || min_count > 0xFFFFFFFEu)
        return kman_fail(ctx, KMAN_EINVAL, "min_count must be in [1, 4294967294], got %u", min_count);
    if (n_bases == 0) return KMAN_OK;
    if (!d_fix) return kman_fail(ctx, KMAN_EINVAL, "kman_correct_sites: null buffer");
    const bool work = n_bases >= k && n_records != 0;
    if (work) {
        if (!d_codes || !d_wc || !d_rec_seq || !d_index || (nt && (!d_tkeys || !d_tcounts)))
            return kman_fail(ctx, KMAN_EINVAL, "kman_correct_sites: null buffer");
        if (((uintptr_t)d_wc & 15) != 0) return kman_fail(ctx, KMAN_EINVAL, "d_wc must be 16-byte aligned");
    }
    const uint64_t tiles = ceil_div(n_bases, CTILE);
    if (tiles > 0x7ffffffeull || n_records > (~0ull >> 5))
        return kman_fail(ctx, KMAN_EINVAL, "%llu bases, %llu records: too many", (unsigned long long)n_bases,
                         (unsigned long long)n_records);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    void *d_n = nullptr;
    if (work) KMAN_TRY(kman_scratch(ctx, 16, &d_n));
    HIP_TRY(ctx, hipMemsetAsync(d_fix, 0xFF, (size_t)n_bases, ctx->stream));
    unsigned long long n = 0;
    if (work) {
        HIP_TRY(ctx, hipMemsetAsync(d_n, 0, 16, ctx->stream));
        const uint32_t shift = 2 * k - index_bits;
        {
            KTimer kt_(ctx, "correct_sites");
            if (flags & KMAN_CANONICAL) {
                if (t_count_bytes == 4)
                    launch_correct_sites<1, uint32_t>(ctx, d_codes, n_bases, k, d_wc, d_rec_seq, n_records, d_tkeys,
                                                      d_tcounts, nt, d_index, shift, min_count, d_fix,
                                                      (unsigned long long *)d_n, tiles);
                else
                    launch_correct_sites<1, uint64_t>(ctx, d_codes, n_bases, k, d_wc, d_rec_seq, n_records, d_tkeys,
                                                      d_tcounts, nt, d_index, shift, min_count, d_fix,
                                                      (unsigned long long *)d_n, tiles);
            } else {
                if (t_count_bytes == 4)
                    launch_correct_sites<0, uint32_t>(ctx, d_codes, n_bases, k, d_wc, d_rec_seq, n_records, d_tkeys,
                                                      d_tcounts, nt, d_index, shift, min_count, d_fix,
                                                      (unsigned long long *)d_n, tiles);
                else
                    launch_correct_sites<0, uint64_t>(ctx, d_codes, n_bases, k, d_wc, d_rec_seq, n_records, d_tkeys,
                                                      d_tcounts, nt, d_index, shift, min_count, d_fix,
                                                      (unsigned long long *)d_n, tiles);
            }
            HIP_TRY(ctx, hipGetLastError());
        }
        HIP_TRY(ctx, hipMemcpyAsync(&n, d_n, 8, hipMemcpyDeviceToHost, ctx->stream));
    }
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    if (n_fixed) *n_fixed = (uint64_t)n;
    return KMAN_OK;
}

extern "C" int kman_apply_fixes(kman_ctx *ctx, uint8_t *d_codes, uint64_t n_bases, const uint8_t *d_fix,
                                const uint64_t *d_rec_seq, uint64_t n_records, uint8_t *d_text, uint64_t n_bytes,
                                const uint64_t *d_rec_off, uint32_t *d_nfix) {
    if (!ctx) return KMAN_EINVAL;
    if ((n_bases && (!d_codes || !d_fix)) || (n_records && (!d_rec_seq || !d_nfix)) || (d_text && !d_rec_off))
        return kman_fail(ctx, KMAN_EINVAL, "kman_apply_fixes: null buffer");
    if (((uintptr_t)d_fix & 15) != 0 || ((uintptr_t)d_text & 15) != 0)
        return kman_fail(ctx, KMAN_EINVAL, "d_fix and d_text must be 16-byte aligned");
    if (ceil_div(n_bases, 16 * CT_) > 0x7ffffffeull || n_records > (1ull << 31))
        return kman_fail(ctx, KMAN_EINVAL, "%llu bases, %llu records: too many", (unsigned long long)n_bases,
                         (unsigned long long)n_records);
    if (n_bases == 0 && n_records == 0) return KMAN_OK;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    {
        KTimer kt_(ctx, "apply_fixes");
        if (n_records) {
            // (before the codes: neither kernel reads what the other writes)
            hipLaunchKernelGGL(apply_records_kernel, dim3((uint32_t)ceil_div(n_records, CT_ / 64)), dim3(CT_), 0,
                               ctx->stream, d_fix, n_bases, d_rec_seq, n_records, d_text, n_bytes, d_rec_off, d_nfix);
            HIP_TRY(ctx, hipGetLastError());
        }
        if (n_bases) {
            hipLaunchKernelGGL(apply_codes_kernel, dim3((uint32_t)ceil_div(n_bases, 16 * CT_)), dim3(CT_), 0,
                               ctx->stream, d_codes, n_bases, d_fix);
            HIP_TRY(ctx, hipGetLastError());
        }
    }
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return KMAN_OK;
}
