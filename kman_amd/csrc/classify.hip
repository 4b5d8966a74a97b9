// classify.hip — reads among up to 64 references: for every record, how many
// of its k-mer windows are rows of a coloured table, per colour.
//
// The coloured table (engine.color_table) is the union of the references'
// k-mers; the u64 "count" of a row is the mask of the references that hold it,
// bit c for reference c.  kman_classify_records is screen.hip's kernel with
// another reduction: one block of 256 threads per tile of CTILE = 4096
// windows, stage_codes + roll<16, CANON>, then table_lookup<16, uint64_t> with
// the masks as the count array -- ONE lookup per window whatever the number of
// colours; a thread then holds its 16 windows' masks in registers.
//   masks      cut to the bits < n_colors; under KMAN_CLASSIFY_SPECIFIC a mask
//              with more than one bit left becomes 0 (the window counts for a
//              colour only when no other reference holds its k-mer).  After
//              this a window counts for colour c when bit c is set, in both
//              modes.
//   records    as in screen.hip (tile_records.h: cut_slice, stage_slice,
//              owner_walk): <= CCAP slice entries are staged in LDS (one round
//              of slots), more are searched in global memory (CTILE / CCAP
//              rounds of CCAP slots).
//   colours    in chunks of CCH = 8: a chunk holds 8 register counters per run
//              of one record and 8 x CCAP u32 LDS slots.  n_colors <= 8 is one
//              chunk (the MULTI = 0 instances have no chunk loop); 64 colours
//              are eight chunks over masks already in registers.  The OR of
//              the block's masks is gathered in LDS first: a chunk none of
//              whose colours occurs in the tile is skipped by the whole block
//              (chunk 0 always runs: it carries the windows plane), and a
//              thread whose own 16 masks lack the chunk's colours does not
//              walk its windows again.
//   reduction  a run's nonzero counters are u32 atomicAdds to LDS (windows:
//              sw, colours: sc[colour in chunk][slot]), then every nonzero
//              (slot, plane) is one u32 atomicAdd to d_out.  Integer adds
//              commute: the result does not depend on the order.
//
// Bounds, not values: tile_records.h for the records and slots, screen_lookup.h
// for the table; every record that addresses d_out is checked against
// n_records, and the plane index of every global add is 1 + c0 + cc with c0 + cc < n_colors
// checked where it is formed.
//
// kman_classify_pick: one thread per record reads its n_colors hit words
// (plane-major, so a wave reads 256 contiguous bytes per plane) and writes the
// winner, its hits and the runner-up's.
//
// Algorithmic bytes per valid window: screen.hip's (1 B code, one 16 B index
// pair, at most floor(log2 bucket) + 1 random 8 B key reads) and 8 B of mask on
// a hit; per (tile, record): 4 B atomics, one per nonzero plane.
// kman_classify_pick: 4 n_colors B read and 12 B written per record.
#include "common.h"
#include "kmer.h"
#include "screen_lookup.h"
#include "tile_records.h"

namespace {

constexpr int CT = 256;
constexpr int CEI = 16;
constexpr int CTILE = CT * CEI;
constexpr int CCAP = KMAN_SCREEN_REC_CAP;
constexpr int CCH = 8;  // colours per chunk
static_assert(CTILE == KMAN_SCREEN_TILE, "include/kman.h states the tile size");
static_assert(CTILE % CCAP == 0, "the global path's rounds tile the offsets");
static_assert(KMAN_CLASSIFY_MAX_COLORS == 64, "a mask is one u64");
static_assert(KMAN_CLASSIFY_MAX_COLORS % CCH == 0, "whole chunks");
static_assert((KMAN_CLASSIFY_SPECIFIC & (KMAN_CLASSIFY_SPECIFIC - 1)) == 0 && KMAN_CLASSIFY_SPECIFIC != KMAN_CANONICAL,
              "one flag bit of its own");

template <int CANON, int SPEC, int MULTI>
__global__ __launch_bounds__(CT) void classify_kernel(const uint8_t *__restrict__ codes, uint64_t n_bases, int k,
                                                      const uint64_t *__restrict__ rec_seq, uint64_t n_records,
                                                      const uint64_t *__restrict__ tkeys,
                                                      const uint64_t *__restrict__ tmasks, uint64_t nt,
                                                      const uint64_t *__restrict__ index, uint32_t shift,
                                                      uint32_t n_colors, uint32_t *__restrict__ out) {
    __shared__ __attribute__((aligned(16))) uint8_t scodes[CTILE + 64];
    __shared__ uint64_t srec[CCAP];  // LDS path: the slice of rec_seq; global path: the record of each slot
    __shared__ uint32_t sw[CCAP];
    __shared__ uint32_t sc[CCH * CCAP];  // [colour in chunk][slot]
    __shared__ uint64_t s_r0, s_ns;
    __shared__ unsigned long long s_any;  // the OR of the block's masks

    const uint64_t tb = (uint64_t)blockIdx.x * CTILE;
    if (threadIdx.x == 0) {
        const TileSlice s = cut_slice(rec_seq, n_records, tb, umin64(tb + CTILE, n_bases) - 1);
        s_r0 = s.r0;
        s_ns = s.ns;
        s_any = 0;
    }
    stage_codes<CT, CEI>(codes, n_bases, tb, scodes);
    __syncthreads();
    const uint64_t r0 = s_r0, ns = s_ns;
    if (ns == 0) return;  // (no record starts at or before the tile's last base)
    const SliceView sv = stage_slice<CT, CCAP>(rec_seq, {r0, ns, 0}, srec);
    const bool big = sv.big;

    const uint64_t mask = k == 32 ? ~0ull : ((1ull << (2 * k)) - 1);
    uint64_t kf[CEI], kr[CEI];
    const uint64_t p0 = tb + (uint64_t)threadIdx.x * CEI;
    const uint32_t valid = roll<CEI, CANON>(scodes, threadIdx.x * CEI, k, mask, p0, n_bases, kf, kr);

    // ---- lookup: one per window; m[j] = the row's mask (screen_lookup.h)
    uint64_t m[CEI];
    table_lookup<CEI, uint64_t>(valid, kf, shift, index, tkeys, tmasks, nt, m);
    const uint64_t cmask = n_colors >= 64 ? ~0ull : ((1ull << n_colors) - 1);
    uint64_t any = 0;
#pragma unroll
    for (int j = 0; j < CEI; j++) {
        uint64_t x = m[j] & cmask;
        if (SPEC && (x & (x - 1))) x = 0;
        m[j] = x;
        any |= x;
    }
    if (MULTI && any) atomicOr(&s_any, (unsigned long long)any);

    // ---- per-record, per-colour reduction
    struct Run {
        uint32_t h[CCH];
    };
    const int rounds = big ? CTILE / CCAP : 1;
    const uint32_t nchunks = MULTI ? (n_colors + CCH - 1) / CCH : 1;
    for (int c = 0; c < rounds; c++) {
        for (uint32_t ch = 0; ch < nchunks; ch++) {
            const uint32_t c0 = ch * CCH;
            for (uint32_t i = threadIdx.x; i < (uint32_t)CCAP; i += CT) sw[i] = 0;
            for (uint32_t i = threadIdx.x; i < (uint32_t)(CCH * CCAP); i += CT) sc[i] = 0;
            __syncthreads();  // (and, the first time, the slice in srec and s_any)
            // (block-uniform: s_any is complete after the first barrier and is not written again)
            const bool chunk_on = ch == 0 || ((s_any >> c0) & 0xffull) != 0;
            const bool mine = ch == 0 || ((any >> c0) & 0xffull) != 0;
            if (chunk_on && valid && mine)
                owner_walk<CEI, CCAP, Run>(
                    sv, r0, tb, p0, valid, c, srec,
                    [&](Run &a, int j) {
                        const uint32_t bits = (uint32_t)(m[j] >> c0) & 0xffu;
                        if (bits) {
#pragma unroll
                            for (int cc = 0; cc < CCH; cc++) a.h[cc] += (bits >> cc) & 1u;
                        }
                    },
                    [&](const Run &a, uint32_t w, uint32_t slot) {
                        if (ch == 0) atomicAdd(&sw[slot], w);
#pragma unroll
                        for (int cc = 0; cc < CCH; cc++)
                            if (a.h[cc]) atomicAdd(&sc[cc * CCAP + slot], a.h[cc]);
                    });
            __syncthreads();
            if (chunk_on) {
                for (uint32_t i = threadIdx.x; i < (uint32_t)CCAP; i += CT) {
                    const uint32_t wv = ch == 0 ? sw[i] : 0;
                    uint32_t hv[CCH], nz = wv;
#pragma unroll
                    for (int cc = 0; cc < CCH; cc++) {
                        hv[cc] = sc[cc * CCAP + i];
                        nz |= hv[cc];
                    }
                    if (nz == 0) continue;
                    const uint64_t r = big ? srec[i] : r0 + i;
                    if (r >= n_records) continue;  // (cannot happen: r < r0 + ns <= n_records)
                    if (wv) atomicAdd(&out[r], wv);
#pragma unroll
                    for (int cc = 0; cc < CCH; cc++)
                        if (hv[cc] && c0 + cc < n_colors) atomicAdd(&out[(uint64_t)(1 + c0 + cc) * n_records + r], hv[cc]);
                }
            }
            __syncthreads();
        }
    }
}

__global__ __launch_bounds__(256) void classify_pick_kernel(const uint32_t *__restrict__ planes, uint64_t n_records,
                                                            uint32_t n_colors, uint32_t *__restrict__ pick) {
    const uint64_t r = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= n_records) return;
    uint32_t best = planes[n_records + r], bc = 0, second = 0;
    for (uint32_t c = 1; c < n_colors; c++) {
        const uint32_t v = planes[(uint64_t)(1 + c) * n_records + r];
        if (v > best) {
            second = best;
            best = v;
            bc = c;
        } else if (v > second) {
            second = v;
        }
    }
    pick[r] = best ? bc : KMAN_CLASSIFY_NONE;
    pick[n_records + r] = best;
    pick[2 * n_records + r] = second;
}

template <int CANON, int SPEC, int MULTI>
void launch_classify(kman_ctx *ctx, const uint8_t *codes, uint64_t n_bases, uint32_t k, const uint64_t *rec_seq,
                     uint64_t n_records, const uint64_t *tkeys, const uint64_t *tmasks, uint64_t nt,
                     const uint64_t *index, uint32_t shift, uint32_t n_colors, uint32_t *out, uint64_t tiles) {
    hipLaunchKernelGGL((classify_kernel<CANON, SPEC, MULTI>), dim3((uint32_t)tiles), dim3(CT), 0, ctx->stream, codes,
                       n_bases, (int)k, rec_seq, n_records, tkeys, tmasks, nt, index, shift, n_colors, out);
}

}  // namespace

extern "C" int kman_classify_records(kman_ctx *ctx, const uint8_t *d_codes, uint64_t n_bases, uint32_t k,
                                     uint32_t flags, const uint64_t *d_rec_seq, uint64_t n_records,
                                     const uint64_t *d_tkeys, const uint64_t *d_tmasks, uint64_t nt,
                                     const uint64_t *d_index, uint32_t index_bits, uint32_t n_colors,
                                     uint32_t *d_out) {
    if (!ctx) return KMAN_EINVAL;
    if (k < 2 || k > 32) return kman_fail(ctx, KMAN_EINVAL, "k must be in [2, 32] on the GPU path, got %u", k);
    if (flags & ~(KMAN_CANONICAL | KMAN_CLASSIFY_SPECIFIC))
        return kman_fail(ctx, KMAN_EINVAL, "kman_classify_records: flags 0x%x", flags);
    if (n_colors < 1 || n_colors > KMAN_CLASSIFY_MAX_COLORS)
        return kman_fail(ctx, KMAN_EINVAL, "n_colors must be in [1, %d], got %u", KMAN_CLASSIFY_MAX_COLORS, n_colors);
    if (!index_bits_ok(k, index_bits))
        return kman_fail(ctx, KMAN_EINVAL, "index_bits must be in [1, min(2k, %d)], got %u (k = %u)",
                         KMAN_SCREEN_MAX_INDEX_BITS, index_bits, k);
    if (n_records == 0) return KMAN_OK;
    if (!d_out || !d_rec_seq) return kman_fail(ctx, KMAN_EINVAL, "kman_classify_records: null buffer");
    if (n_records > (~0ull >> 2) / (4 * (KMAN_CLASSIFY_MAX_COLORS + 1)))
        return kman_fail(ctx, KMAN_EINVAL, "too many records");
    const bool launch = n_bases >= k;
    if (launch) {  // (a refused call writes nothing: checked before the planes are zeroed)
        if (!d_codes || !d_index || (nt && (!d_tkeys || !d_tmasks)))
            return kman_fail(ctx, KMAN_EINVAL, "kman_classify_records: null buffer");
        if (((uintptr_t)d_codes & 15) != 0) return kman_fail(ctx, KMAN_EINVAL, "codes must be 16-byte aligned");
        if (ceil_div(n_bases, CTILE) > 0x7ffffffeull)
            return kman_fail(ctx, KMAN_EINVAL, "%llu bases: too many tiles", (unsigned long long)n_bases);
    }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipMemsetAsync(d_out, 0, (size_t)(4 * (uint64_t)(1 + n_colors) * n_records), ctx->stream));
    if (launch) {
        const uint64_t tiles = ceil_div(n_bases, CTILE);
        const uint32_t shift = 2 * k - index_bits;
        const int which = ((flags & KMAN_CANONICAL) ? 4 : 0) | ((flags & KMAN_CLASSIFY_SPECIFIC) ? 2 : 0) |
                          (n_colors > (uint32_t)CCH ? 1 : 0);
        KTimer kt_(ctx, "classify");
#define KMAN_CLASSIFY_CASE(w, CANON, SPEC, MULTI)                                                                  \
    case w:                                                                                                         \
        launch_classify<CANON, SPEC, MULTI>(ctx, d_codes, n_bases, k, d_rec_seq, n_records, d_tkeys, d_tmasks, nt, \
                                            d_index, shift, n_colors, d_out, tiles);                               \
        break;
        switch (which) {
            KMAN_CLASSIFY_CASE(0, 0, 0, 0)
            KMAN_CLASSIFY_CASE(1, 0, 0, 1)
            KMAN_CLASSIFY_CASE(2, 0, 1, 0)
            KMAN_CLASSIFY_CASE(3, 0, 1, 1)
            KMAN_CLASSIFY_CASE(4, 1, 0, 0)
            KMAN_CLASSIFY_CASE(5, 1, 0, 1)
            KMAN_CLASSIFY_CASE(6, 1, 1, 0)
            KMAN_CLASSIFY_CASE(7, 1, 1, 1)
        }
#undef KMAN_CLASSIFY_CASE
        HIP_TRY(ctx, hipGetLastError());
    }
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return KMAN_OK;
}

extern "C" int kman_classify_pick(kman_ctx *ctx, const uint32_t *d_planes, uint64_t n_records, uint32_t n_colors,
                                  uint32_t *d_pick) {
    if (!ctx) return KMAN_EINVAL;
    if (n_colors < 1 || n_colors > KMAN_CLASSIFY_MAX_COLORS)
        return kman_fail(ctx, KMAN_EINVAL, "n_colors must be in [1, %d], got %u", KMAN_CLASSIFY_MAX_COLORS, n_colors);
    if (n_records == 0) return KMAN_OK;
    if (!d_planes || !d_pick) return kman_fail(ctx, KMAN_EINVAL, "kman_classify_pick: null buffer");
    if (n_records > (~0ull >> 2) / (4 * (KMAN_CLASSIFY_MAX_COLORS + 1)))
        return kman_fail(ctx, KMAN_EINVAL, "too many records");
    const uint64_t blocks = ceil_div(n_records, 256);
    if (blocks > 0x7ffffffeull) return kman_fail(ctx, KMAN_EINVAL, "too many records");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    {
        KTimer kt_(ctx, "classify_pick");
        hipLaunchKernelGGL(classify_pick_kernel, dim3((uint32_t)blocks), dim3(256), 0, ctx->stream, d_planes, n_records,
                           n_colors, d_pick);
        HIP_TRY(ctx, hipGetLastError());
    }
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return KMAN_OK;
}
