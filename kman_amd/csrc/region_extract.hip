// region_extract.hip — pass 0 of the region path (region.h): rg_extract, the
// shard histogram rg_hist in the same tile geometry, and their launchers.
#include "region.h"
#include "kmer.h"
#include "onesweep.h"

using namespace kman::region;

namespace {

// ---------------------------------------------------------------- pass 0
// A tile of RT*EI window starts: windows rolled from LDS-staged codes and
// ranked straight from the roll's registers by one block-wide LDS atomic per
// item on the top 8 key bits (item i = window i, or 2j / 2j + 1 = window j's
// two strands with RC; tile-local (window << 1 | strand) packed above the 2k
// key bits), LDS-staged coalesced scatter into region (b, s).
// A tile takes its place in region (b, s) by one atomic add per digit on the
// region's cursor (cursor[s * 256 + b], zeroed before the launch; it ends as the
// region's count), issued right after the rank so its round trip overlaps the
// digit scan and the LDS scatter.  A region's items are then in no particular
// order, which nothing downstream needs: pass 1 ranks unstably and the finish
// sorts every remaining key bit (uniq items carry their window index, so
// equal keys are dropped or counted whatever their order).  No tile waits on
// another tile.
// Segment s of a tile:
//   kman_groups (IL = !EX): interleaved chains -- tile t is in segment t % RS,
//     so any prefix of the stream spreads over every segment and pass 0 can
//     run in consecutive launches over tile ranges as the codes arrive
//     (kman_groups_extract: the epoch's ticket counter carries on from one
//     launch to the next, and a launch of n blocks takes the next n tiles);
//   EX (the multi-GPU shard path, kman_dshard_extract): contiguous runs of
//     seg_tiles tiles, rg_hist's geometry; no padded regions -- region (b, s)
//     is written at rtab[b * RS + s] (exact sizes from rg_hist in cnt0, which
//     is read-only); buckets with rtab == ~0 are not kept this round, and
//     their windows are dropped before the rank (keep bitmap).
// XG (a whole-stream launch): tiles by XCD partition -- segments
// [p * RS / 8, (p + 1) * RS / 8) form partition p, whose tiles the blocks on
// XCD p take in stream order (block id -> tile, no ticket).  So the tiles
// that claim consecutive slots of a region usually run on one XCD: the
// 128-byte line two of them share meets in that XCD's L2 instead of leaving
// two partial lines.  Placement changes only speed.
template <int EI, bool RC, int CANON, bool EX, bool XG, int P0B = (int)(EX ? B1 : G1)>
__global__ __launch_bounds__(RT, (RC ? (EI == 6 ? 6 : 4) : (EI == 12 ? 6 : (EI == 8 ? 8 : 4)))) void rg_extract(
    const uint8_t *__restrict__ codes, uint64_t n_bases, int k, uint32_t Q, uint64_t *__restrict__ out, uint64_t C0,
    uint32_t seg_tiles, uint32_t n_tiles, const uint32_t *__restrict__ cnt0, uint32_t *__restrict__ cursor,
    uint32_t *__restrict__ counter, uint32_t *__restrict__ err, uint64_t *__restrict__ stp,
    const uint64_t *__restrict__ rtab) {
    constexpr int NT = RT;
    constexpr int NWAVE = NT / 64;
    constexpr int WIN = NT * EI;
    constexpr int TILE = WIN * (RC ? 2 : 1);
    constexpr int SI = TILE / NT;
    constexpr bool IL = !EX;
    static_assert(WIN + 64 <= TILE * 8, "codes fit in the key staging area");
    static_assert(RS % 8 == 0, "XCD partitions of whole segments");
    constexpr uint32_t R0 = 1u << P0B;  // pass-0 radix
    static_assert(R0 <= (uint32_t)NT && (!EX || R0 == RADIX), "a thread per digit; the round path's 256 buckets");
    __shared__ __attribute__((aligned(16))) uint64_t skeys[TILE];
    __shared__ uint32_t thist[R0];
    __shared__ uint32_t lstart[R0];
    // !EX: the output index of the tile's item q (a digit-d item) is
    // gexcl[d] + q, stored when q < qlim[d] (the items past a region's
    // capacity are not).  EX: gexcl[d] + q - lstart[d], ~0 for a digit not
    // kept (the !EX form measured slower there: config 4's extraction 87 vs
    // 75 ms, `r04x_extract_ex_ab.txt`)
    __shared__ uint64_t gexcl[R0];
    __shared__ uint32_t qlim[EX ? 1 : R0];
    __shared__ uint32_t lds_scan[NWAVE];
    __shared__ uint32_t keep[EX ? R0 / 32 : 1];

    // one tile per block: the block's tile (XG: from the block id), or a
    // ticket (thread 0 only); ~0u past the tiles / a segment's end.  (Persistent blocks that load the next tile's codes
    // into registers while this one is worked measured slower: 3.97-4.19 vs
    // 3.64-3.83 ms, the loop costs registers and spills.)
    __shared__ uint32_t lds_tile;
    auto take = [&]() -> uint32_t {
        uint32_t c = ~0u;
        if (XG) {
            // block b runs on XCD b % 8 (workgroups are dealt to the XCDs
            // round robin): within each 64 blocks, b = 8 c + x takes tile
            // 8 x + c, so XCD x works through the segments of partition x in
            // stream order.  (Tickets from a per-partition atomic counter,
            // the XCD read from HW_REG_XCC_ID, cost a round trip before the
            // codes load: 2.92 vs 2.75 ms, config 4's extraction 75.4 vs 68.7
            // ms, `r04ad_static_tiles_ab.txt`)
            const uint32_t b = blockIdx.x;
            c = (b & ~63u) | ((b & 7u) << 3) | ((b >> 3) & 7u);
        } else {
            c = atomicAdd(counter, 1u);
        }
        if (c == ~0u) return ~0u;
        if (IL) return c < n_tiles ? c : ~0u;
        const uint32_t s_ = c % RS, jj = c / RS, t0 = s_ * seg_tiles;
        return t0 + jj < (t0 + seg_tiles < n_tiles ? t0 + seg_tiles : n_tiles) ? c : ~0u;
    };
    uint32_t cid;
    if (XG) {
        cid = take();  // (block-uniform)
    } else {
        if (threadIdx.x == 0) lds_tile = take();
        __syncthreads();
        cid = lds_tile;
    }
    if (cid == ~0u) return;  // (block-uniform)
    const int64_t tile = IL ? (int64_t)cid : (int64_t)(cid % RS) * seg_tiles + cid / RS;
    const uint32_t sgi = cid % RS;
    RSTAMP(tile, 0);
    const uint32_t kb = 2u * (uint32_t)k;
    const uint32_t shift = kb - P0B;
    const uint64_t keymask = kb >= 64 ? ~0ull : ((1ull << kb) - 1);
    const uint64_t restmask = (1ull << shift) - 1;
    uint8_t *scodes = reinterpret_cast<uint8_t *>(skeys);
    const uint64_t wb = (uint64_t)tile * WIN;
    // wave priority 2 while the tile's codes load and its items store, 0 for
    // the roll and rank: the memory phases go ahead of the other blocks'
    // compute (config 4's shard extraction 62.3 -> 60.2 ms; the 1 GB
    // extraction unchanged, `r04ap_xprio_ab.txt`)
    __builtin_amdgcn_s_setprio(2);
    stage_codes<NT, EI>(codes, n_bases, wb, scodes);
    if (threadIdx.x < R0) thist[threadIdx.x] = 0;
    // EX: thread d < R0 holds region (d, sgi)'s table entry and exact size
    // from here on (loaded with the codes, not behind the cursor atomic:
    // config 4's extraction 67.3 -> 62.5 ms, `r04ag_ex_prefetch_ab.txt`)
    uint64_t rb_d = ~0ull;
    uint32_t cnt_d = 0;
    if (EX && threadIdx.x < R0) {  // (one table load per thread, a ballot per wave)
        rb_d = rtab[(uint64_t)threadIdx.x * RS + sgi];
        cnt_d = cnt0[threadIdx.x * RS + sgi];
        const uint64_t bal = __ballot(rb_d != ~0ull);
        if ((threadIdx.x & 63) == 0) {
            keep[threadIdx.x / 32] = (uint32_t)bal;
            keep[threadIdx.x / 32 + 1] = (uint32_t)(bal >> 32);
        }
    }
    __syncthreads();
    RSTAMP(tile, 1);
    __builtin_amdgcn_s_setprio(0);

    uint64_t kf[EI], kr[EI];
    const uint32_t w0 = threadIdx.x * EI;
    // (CANON: kf = min(forward, reverse complement), one key per window)
    const uint32_t valid = roll<EI, CANON>(scodes, w0, k, keymask, wb + w0, n_bases, kf, kr);
    uint32_t vf = valid, vr = RC ? valid : 0u;
    if (EX) {  // only the buckets kept this round
#pragma unroll
        for (int j = 0; j < EI; j++) {
            const uint32_t df = (uint32_t)(kf[j] >> shift);
            vf &= ~((uint32_t)!((keep[df >> 5] >> (df & 31)) & 1u) << j);
            if (RC) {
                const uint32_t dr = (uint32_t)(kr[j] >> shift);
                vr &= ~((uint32_t)!((keep[dr >> 5] >> (dr & 31)) & 1u) << j);
            }
        }
    }
    uint64_t key[SI];
    uint32_t rank[SI];
    uint32_t vmask = 0;    // item i of this thread is valid
    uint32_t at_base = 0;  // this tile's first slot in region (d, sgi), thread d
#define XDIGIT(x) ((uint32_t)(((x) & keymask) >> shift))
    // the tile-local (window << 1 | strand) rides above the key bits: only
    // uniq items carry it (Q > 0, k <= 25); count items are the key
    auto tagged = [&](int j, bool strand) -> uint64_t {
        return Q ? (uint64_t)(((w0 + j) << 1) | (uint32_t)strand) << kb : 0ull;
    };
#pragma unroll
    for (int j = 0; j < EI; j++) {
        if (RC) {
            key[2 * j] = kf[j] | tagged(j, false);
            key[2 * j + 1] = kr[j] | tagged(j, true);
            vmask |= (((vf >> j) & 1u) << (2 * j)) | (((vr >> j) & 1u) << (2 * j + 1));
        } else {
            key[j] = kf[j] | tagged(j, false);
        }
    }
    if (!RC) vmask = vf;
#pragma unroll
    for (int i = 0; i < SI; i++) rank[i] = (vmask >> i) & 1u ? atomicAdd(&thist[XDIGIT(key[i])], 1u) : 0u;
    __syncthreads();  // (also: every roll read of the staged codes before the scatter below)
    RSTAMP(tile, 2);
    if (threadIdx.x < R0) {  // the tile's place in each region, claimed now
        const uint32_t c = thist[threadIdx.x];
        // (cursor[s * 256 + b]: a wave's 64 adds are 256 contiguous bytes,
        // which leave L2 as four 64-byte requests to the memory-side atomic
        // units -- at cursor[b * RS + s] they were 64 requests, one per lane)
        at_base = c ? atomicAdd(cursor + (uint64_t)sgi * R0 + threadIdx.x, c) : 0u;
    }
    RSTAMP(tile, 3);
    const uint32_t d0 = threadIdx.x;
    const uint32_t tot = d0 < R0 ? thist[d0] : 0u;
    uint32_t tcnt;
    const uint32_t ls = block_exclusive_scan1<NT>(tot, SumU32(), 0u, lds_scan, &tcnt);
    if (d0 < R0) lstart[d0] = ls;
    __syncthreads();
    // (the slot reads issued first, back to back, then the writes: 3.23 vs
    // 3.12 ms, the same with the store loop's reads -- `r04o_pipe_ab.txt`)
#pragma unroll
    for (int i = 0; i < SI; i++)
        if ((vmask >> i) & 1u) skeys[lstart[XDIGIT(key[i])] + rank[i]] = key[i];

    if (threadIdx.x < R0) {
        const uint32_t d = threadIdx.x, ls = lstart[d], c = thist[d];
        const uint64_t incl = (uint64_t)at_base + c;
        if (EX) {  // (digits not kept this round have no items)
            const uint64_t rb = rb_d;
            const bool over = c && incl > cnt_d;
            if (over && rb != ~0ull) atomicOr(err, ERR_REGION);  // (the input changed under the plan)
            gexcl[d] = rb == ~0ull || over ? ~0ull : rb + at_base;
        } else {
            gexcl[d] = ((uint64_t)d * RS + sgi) * C0 + at_base - ls;
            qlim[d] = ls + (incl <= C0 ? c : at_base < C0 ? (uint32_t)(C0 - at_base) : 0u);
            if (incl > C0) atomicOr(err, ERR_REGION);
        }
    }
    __syncthreads();
    RSTAMP(tile, 4);
    __builtin_amdgcn_s_setprio(2);
    // vmcnt(0) once, on every path: the region-cursor atomic's return (issued
    // only by the waves of threads < R0) is otherwise still pending, as far
    // as the compiler can tell, in the waves that skipped it, and it puts a
    // vmcnt(0) before every store below -- each store waiting for the last
    __builtin_amdgcn_s_waitcnt(0x0f70);
    constexpr int RQ = (TILE + NT - 1) / NT;
#pragma unroll
    for (int r = 0; r < RQ; r++) {
        const uint32_t q = threadIdx.x + r * NT;
        if (q < tcnt) {
            const uint64_t kk = skeys[q];
            const uint32_t d = XDIGIT(kk);
            if (!EX && q >= qlim[d]) continue;
            uint64_t v = kk & restmask;
            if (Q) {
                const uint64_t f = kk >> kb;  // tile-local (window << 1 | strand)
                const uint64_t win = wb + (f >> 1);
                const uint64_t idx = RC ? ((win << 1) | (f & 1u)) : win;
                v = (v << Q) | idx;
            }
            if (EX) {
                if (gexcl[d] != ~0ull) out[gexcl[d] + (q - lstart[d])] = v;
            } else {
                out[gexcl[d] + q] = v;
            }
        }
    }
    RSTAMP(tile, 5);
#undef XDIGIT
}

constexpr uint32_t HIST_BLOCKS_PER_SEG = 32;

// exact (bucket, segment) counts of rg_extract's items: block (j, s) rolls
// the tiles j, j + J, ... of segment s.  The counters are lane-private: lane l
// of every wave adds to column l mod 32 of a [bucket][32] table, so the 32
// lanes of a ds_add lane group hit 32 distinct banks whatever their buckets
// (per-wave [bucket] tables: 4.80 vs 4.36 ms per 12.5 G bases with roll_top,
// `r05mn_hist_ab.txt`)
template <int EI, bool RC, int CANON>
__global__ __launch_bounds__(RT) void rg_hist(const uint8_t *__restrict__ codes, uint64_t n_bases, int k,
                                             uint32_t seg_tiles, uint32_t n_tiles, uint32_t *__restrict__ hist) {
    constexpr int NT = RT, WIN = NT * EI;
    __shared__ __attribute__((aligned(16))) uint8_t scodes[WIN + 64];
    __shared__ uint32_t wh[RADIX * 32];
    const uint32_t col = threadIdx.x & 31u;
    const uint32_t sgi = blockIdx.y;
    const uint32_t t0 = sgi * seg_tiles;
    const uint32_t t1 = t0 + seg_tiles < n_tiles ? t0 + seg_tiles : n_tiles;
    for (int i = threadIdx.x; i < RADIX * 32; i += NT) wh[i] = 0;
    const uint32_t kb = 2u * (uint32_t)k, shift = kb - B1;
    const uint64_t keymask = kb >= 64 ? ~0ull : ((1ull << kb) - 1);
    const uint32_t w0 = threadIdx.x * EI;
    // the next tile's codes are loaded into registers while this tile rolls:
    // one 8 KiB tile per block in flight alone leaves the CU ~24 KiB of reads
    // to hide HBM latency with
    CodeVecs<NT, EI> cv;
    uint32_t t = t0 + blockIdx.x;
    if (t < t1) load_codes<NT, EI>(codes, n_bases, (uint64_t)t * WIN, cv);
    for (; t < t1; t += gridDim.x) {
        const uint64_t wb = (uint64_t)t * WIN;
        __syncthreads();  // the previous tile's rolls read scodes
        store_codes<NT, EI>(cv, codes, n_bases, wb, scodes);
        if (t + gridDim.x < t1) load_codes<NT, EI>(codes, n_bases, (uint64_t)(t + gridDim.x) * WIN, cv);
        __syncthreads();
        if constexpr (!CANON && EI % 4 == 0) {
            // only the keys' top bytes: roll_top, a third of the full roll's
            // VALU work (the full roll made this kernel VALU-bound: 8.4 vs 4.4
            // ms per 12.5 G bases)
            constexpr int A = EI % 16 == 0 ? 16 : (EI % 8 == 0 ? 8 : 4);
            uint32_t bf[EI], br[EI];
            const uint32_t valid = roll_top<EI, RC, A>(scodes, (int)w0, k, wb + w0, n_bases, bf, br);
#pragma unroll
            for (int j = 0; j < EI; j++) {
                if ((valid >> j) & 1u) {
                    atomicAdd(&wh[bf[j] * 32u + col], 1u);
                    if (RC) atomicAdd(&wh[br[j] * 32u + col], 1u);
                }
            }
        } else {
            uint64_t kf[EI], kr[EI];
            const uint32_t valid = roll<EI, CANON>(scodes, w0, k, keymask, wb + w0, n_bases, kf, kr);
#pragma unroll
            for (int j = 0; j < EI; j++) {
                if ((valid >> j) & 1u) {
                    atomicAdd(&wh[(uint32_t)(kf[j] >> shift) * 32u + col], 1u);
                    if (RC) atomicAdd(&wh[(uint32_t)(kr[j] >> shift) * 32u + col], 1u);
                }
            }
        }
    }
    __syncthreads();
    for (uint32_t d = threadIdx.x; d < (uint32_t)RADIX; d += NT) {
        uint32_t c = 0;
        // (column (c + d) mod 32: the lanes of a read spread over the banks)
#pragma unroll 8
        for (uint32_t q = 0; q < 32; q++) c += wh[d * 32u + ((q + d) & 31u)];
        if (c) atomicAdd(&hist[d * RS + sgi], c);
    }
}

// pass 0 over the whole stream (n_launch = 0: tickets per XCD partition) or
// over the next n_launch tiles (the chunked loader: one global ticket
// counter that carries the tile across launches)
template <int EI, bool RC, int CANON = 0>
void launch_extract(kman_ctx *ctx, const RegionPlan &p, const uint8_t *codes, uint64_t n_bases, uint32_t k,
                    uint64_t *r0, uint32_t *c0, uint32_t epoch, uint32_t *counter, uint64_t *stp,
                    uint32_t n_launch) {
    if (!n_launch)
        hipLaunchKernelGGL((rg_extract<EI, RC, CANON, false, true>),
                           dim3((p.n_tiles0 + RS - 1) / RS * RS), dim3(RT), 0, ctx->stream, codes,
                           n_bases, (int)k, p.Q, r0, p.C0, p.seg_tiles, p.n_tiles0, c0, c0,
                           ctx->d_xcounters + 8 * (epoch & 63u), ctx->d_err, stp, nullptr);
    else
        hipLaunchKernelGGL((rg_extract<EI, RC, CANON, false, false>), dim3(n_launch), dim3(RT), 0, ctx->stream, codes,
                           n_bases, (int)k, p.Q, r0, p.C0, p.seg_tiles, p.n_tiles0, c0, c0, counter, ctx->d_err, stp,
                           nullptr);
}

template <int EI, bool RC, int CANON>
void launch_hist(kman_ctx *ctx, const RegionPlan &p, const uint8_t *codes, uint64_t n_bases, uint32_t k,
                 uint32_t *hist) {
    const uint32_t gx = p.seg_tiles < HIST_BLOCKS_PER_SEG ? p.seg_tiles : HIST_BLOCKS_PER_SEG;
    hipLaunchKernelGGL((rg_hist<EI, RC, CANON>), dim3(gx, RS), dim3(RT), 0, ctx->stream, codes, n_bases, (int)k,
                       p.seg_tiles, p.n_tiles0, hist);
}

template <int EI, bool RC, int CANON>
void launch_extract_ex(kman_ctx *ctx, const RegionPlan &p, const uint8_t *codes, uint64_t n_bases, uint32_t k,
                       uint64_t *out, const uint32_t *cnt, const uint64_t *rtab, uint32_t epoch) {
    const uint32_t grid = RS * p.seg_tiles;
    (void)hipMemsetAsync(ctx->d_cursors, 0, (size_t)RADIX * RS * 4, ctx->stream);  // (errors: the caller's hipGetLastError)
    hipLaunchKernelGGL((rg_extract<EI, RC, CANON, true, true>), dim3(grid), dim3(RT), 0, ctx->stream, codes, n_bases,
                       (int)k, p.Q, out, (uint64_t)0, p.seg_tiles, p.n_tiles0, cnt, ctx->d_cursors,
                       ctx->d_xcounters + 8 * (epoch & 63u), ctx->d_err, nullptr, rtab);
}

}  // namespace

void kman::region::launch_extract_any(kman_ctx *ctx, const RegionPlan &p, const uint8_t *codes, uint64_t n_bases,
                                      uint32_t k, uint64_t *r0, uint32_t *c0, uint32_t epoch, uint32_t *counter,
                                      uint64_t *stp, uint32_t n_launch) {
    if (p.canon && p.mix) launch_extract<16, false, 2>(ctx, p, codes, n_bases, k, r0, c0, epoch, counter, stp, n_launch);
    else if (p.canon) launch_extract<16, false, 1>(ctx, p, codes, n_bases, k, r0, c0, epoch, counter, stp, n_launch);
    else if (p.rc) launch_extract<8, true>(ctx, p, codes, n_bases, k, r0, c0, epoch, counter, stp, n_launch);
    else launch_extract<16, false>(ctx, p, codes, n_bases, k, r0, c0, epoch, counter, stp, n_launch);
}

void kman::region::launch_hist_any(kman_ctx *ctx, const RegionPlan &p, const uint8_t *codes, uint64_t n_bases,
                                   uint32_t k, uint32_t *hist) {
    if (p.ei == 16 || p.ei == 8) {
        if (p.canon && p.mix) launch_hist<16, false, 2>(ctx, p, codes, n_bases, k, hist);
        else if (p.canon) launch_hist<16, false, 1>(ctx, p, codes, n_bases, k, hist);
        else if (p.rc) launch_hist<8, true, 0>(ctx, p, codes, n_bases, k, hist);
        else launch_hist<16, false, 0>(ctx, p, codes, n_bases, k, hist);
    } else if (p.canon && p.mix) launch_hist<12, false, 2>(ctx, p, codes, n_bases, k, hist);
    else if (p.canon) launch_hist<12, false, 1>(ctx, p, codes, n_bases, k, hist);
    else if (p.rc) launch_hist<6, true, 0>(ctx, p, codes, n_bases, k, hist);
    else launch_hist<12, false, 0>(ctx, p, codes, n_bases, k, hist);
}

void kman::region::launch_extract_ex_any(kman_ctx *ctx, const RegionPlan &p, const uint8_t *codes, uint64_t n_bases,
                                         uint32_t k, uint64_t *out, const uint32_t *cnt, const uint64_t *rtab,
                                         uint32_t epoch) {
    if (p.ei == 16 || p.ei == 8) {
        if (p.canon && p.mix) launch_extract_ex<16, false, 2>(ctx, p, codes, n_bases, k, out, cnt, rtab, epoch);
        else if (p.canon) launch_extract_ex<16, false, 1>(ctx, p, codes, n_bases, k, out, cnt, rtab, epoch);
        else if (p.rc) launch_extract_ex<8, true, 0>(ctx, p, codes, n_bases, k, out, cnt, rtab, epoch);
        else launch_extract_ex<16, false, 0>(ctx, p, codes, n_bases, k, out, cnt, rtab, epoch);
    } else if (p.canon && p.mix) launch_extract_ex<12, false, 2>(ctx, p, codes, n_bases, k, out, cnt, rtab, epoch);
    else if (p.canon) launch_extract_ex<12, false, 1>(ctx, p, codes, n_bases, k, out, cnt, rtab, epoch);
    else if (p.rc) launch_extract_ex<6, true, 0>(ctx, p, codes, n_bases, k, out, cnt, rtab, epoch);
    else launch_extract_ex<12, false, 0>(ctx, p, codes, n_bases, k, out, cnt, rtab, epoch);
}
