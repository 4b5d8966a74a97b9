// region.hip — `kmer count` / `kmer uniq` of one FASTA stream in three
// kernels, through padded regions of packed items (kman_groups).
//
// Replaces, for one device-resident batch stream, the whole chain
//   Sequence.yield_kmers (kmermaid/seq.py:285-328) -> Batch.sorted
//   (batch.py:156-168, forced by batcher.py:392) -> Crawler.do_records /
//   do_batch (join.py:63-130) -> join_sequence_count / join_unique
//   (join.py:244-285)
// for the inputs whose shape allows it (uniform-ish prefix distribution, k <=
// 25; anything else returns KMAN_EFALLBACK and the caller runs
// kman_extract_sorted + kman_finish, which handle every input).
//
// MSD instead of the LSD prefix passes of sort.hip:
//   pass 0 (rg_extract)  rolls the windows of a tile and scatters them by the
//                        top 8 key bits b into region (b, s) of capacity C0,
//                        s = one of RS position segments (own look-back
//                        chains).  b is implied by the region from here on, so
//                        an item is ONE u64: (key minus its top 8 bits) << Q |
//                        window index (Q bits; Q = 0 in count mode).
//   pass 1 (rg_pass)     per bucket b (its own chain over the regions (b, *)):
//                        scatter by the next B2 key bits d into region
//                        r = (b << B2 | d) of capacity C1 <= FCAP.
//   finish (rg_finish)   one 512-thread block per region r: load it (<= FCAP
//                        items, 68 KiB of LDS), LSD-sort the remaining key
//                        bits in LDS, run-length pass, emit (key, count) or the
//                        keys that occur once with their pos, compacted by one
//                        look-back over the regions in key order.
// No digit histogram is computed before any pass: every region has a fixed
// capacity (1.5x its expected fill), the passes publish their final region
// counts themselves, and a region that would overflow raises a device flag
// (nothing is written past a capacity) that turns the call into
// KMAN_EFALLBACK.  Algorithmic HBM bytes per k-mer: 1 code read + 8 (pass 0)
// + 16 (pass 1) + 8 (finish read) + the output, against 13 + 2 x 24 + 12 for
// the LSD pipeline of the same workload.
#include "common.h"
#include "kmer.h"
#include "onesweep.h"

#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>

namespace {

constexpr int RT = 512;           // threads of passes 0 and 1
constexpr int RS = 64;            // position segments of pass 0 (one wave of counts)
constexpr int RSI = 16;           // items per thread, pass 1
constexpr uint64_t T1 = (uint64_t)RT * RSI;  // pass-1 tile
constexpr int FT = 512;           // finish threads (more threads per region: 640 or 576 -- a second
                                  // block no longer fits the CU's SIMDs, 9.5 / 11.5 vs 5.7 ms; 768,
                                  // two blocks at 80 VGPRs -- 6.7 ms, the sort phase's barriers over
                                  // 12 waves cost more than the waves gain)
constexpr int FCAP = 8704;        // finish capacity: 68 KiB of 8-byte items
constexpr int FBITS = 9;          // finish LSD digit (26 bits: 3 passes)
constexpr int FRAD = 1 << FBITS;
constexpr int FWORD = FRAD / 2;   // per-wave counters: two u16 per word
constexpr uint32_t ERR_REGION = 1u << 8;  // a region would overflow (not an engine fault)
constexpr uint32_t ERR_EARLY = 1u << 9;   // the uniq finish's early row count was not its rows'
constexpr uint32_t B1 = 8;        // pass-0 digit: top 8 key bits
// kman_groups' pass-0 bits.  (9, with 9 more in pass 1, leaves regions of ~3.8
// K items per 1 G k-mers that a GCAP finish holds in 40 KiB -- three blocks
// per CU -- but the finish's per-region costs dominate there: 5.96 vs 5.62
// ms, and the 512-bucket pass 0 4.0 vs 3.6 ms)
// (Round 5, with the cursor adds cheap: 9 + 8 bits measured equal to 8 + 9,
// `r05xy_pass_geometry_ab.txt`)
#ifndef KMAN_G1
#define KMAN_G1 8
#endif
constexpr uint32_t G1 = KMAN_G1;
// finish capacities (items): FCAP (68 KiB of 8-byte items, two blocks per
// CU) and GCAP (40 KiB, three blocks per CU) for the round path's small
// regions (a pass 1b over many ranks' items leaves ~4 K per region)
constexpr int GCAP = 5120;
// expected region fills the plans aim at (<= T) and accept (<= M): M keeps
// > 10 sd of a uniform fill below the capacity
constexpr uint64_t FFILL_T = 6144, FFILL_M = 7800;

// phase stamps (s_memrealtime, 100 MHz) per tile, thread 0, into `stp`: only
// in diagnostic builds (make EXTRA=-DKMAN_RG_STAMPS OUT=../lib_stamps,
// tools/regionstamps.py); `stp` is null otherwise
#ifdef KMAN_RG_STAMPS
#define RSTAMP(id, i)                                                                                 \
    do {                                                                                              \
        if (stp && threadIdx.x == 0) stp[(uint64_t)(id) * 16 + (i)] = __builtin_amdgcn_s_memrealtime(); \
    } while (0)
#else
#define RSTAMP(id, i) \
    do {              \
        (void)stp;    \
    } while (0)
#endif

KMAN_DEV uint32_t ballot_rank(uint32_t *hist, uint32_t d, bool valid, uint32_t bits) {
    // stable in-wave rank among equal digits (ballot match-any), lane order
    const int lane = lane_id();
    uint64_t peers = __ballot(valid);
    for (uint32_t b = 0; b < bits; b++) {
        const bool set = (d >> b) & 1u;
        const uint64_t m = __ballot(set);
        peers &= set ? m : ~m;
    }
    uint32_t before = 0;
    if (valid) before = hist[d];
    const uint32_t r = before + (uint32_t)__popcll(peers & lanemask_lt());
    const int leader = __ffsll((unsigned long long)peers) - 1;
    if (valid && lane == leader) hist[d] = before + (uint32_t)__popcll(peers);
    return r;
}

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

// ---------------------------------------------------------------- pass 1
// The input of a digit pass: nbk buckets, each the concatenation of nsg <= 64
// segments (bucket bk, segment s: seg_cnt[bk * nsg + s] items at seg_base[..],
// or at (bk * nsg + s) * stride when seg_base is null).  Digit = item bits
// [shift, shift + bits), bits <= 9.  Output region of digit d: ((bk / gsub)
// << bits | d) * gsub + bk % gsub (gsub > 1 keeps the sub-buckets' outputs
// apart, as sub-regions of one region), split into H sub-regions (one per
// chain of the bucket) of capacity C1.  With tag, bits [tag_shift, tag_shift +
// tag_bits) of each item are replaced by its segment index / tag_div as it is
// loaded (the source rank on N > 1).
constexpr int R1 = 512;  // pass-1 radix bound
struct PassArgs {
    const void *in;  // items of TI (rg_pass's template): 8 bytes, or 4 (narrow count items)
    const uint64_t *seg_base;
    const uint32_t *seg_cnt;
    uint32_t cnt_sb;  // seg_cnt indexed [segment][bucket] (pass 0's cursors), else [bucket][segment]
    uint64_t stride;
    uint32_t nbk, nsg, gsub, maxt;
    uint32_t H;        // chains (parts) per bucket: outputs are H sub-regions per region
    uint32_t tag_div;  // tag = segment index / tag_div
    uint32_t shift, bits;
    uint32_t tag, tag_shift, tag_bits;
    void *out;  // items of TO
    uint64_t C1;
    uint32_t *cnt1;
    // optional: a sub-region that overflows C1 flags the finish regions
    // [(sub / fail_div) << fail_shift, +2^fail_shift) in fail[] (the round
    // path then leaves them out and redoes only their keys)
    uint8_t *fail;
    uint32_t fail_div, fail_shift;
    uint32_t big;  // a pass of <= 8 bits on the 1024-thread instance anyway (8192-item tiles: 256-byte digit runs)
    // 8-byte items on that instance without a staged tile, through 256-byte
    // lines (rg_pass<..., LN = true>; kman_groups); line1 (KMAN_PASS_LINE1, for
    // tests): one line per digit at any digit width, so that small inputs take
    // many placement rounds per tile
    uint32_t lines, line1;
    // optional (pass 1 of a key round, rg_pass<..., HV = true): the heavy
    // keys of the round, per bucket j of the round an open-addressing table
    // of HV_BSLOTS key rests (the item's key bits, item >> hv_q; HV_EMPTY
    // where free) at hv_tab[j * HV_BSLOTS], copied to LDS when a chain of
    // the bucket starts (a bucket holds <= HV_BMAX of them).  An item whose
    // key rest is in it is counted per slot in LDS; count mode keeps the
    // chain's first copy (hv_keep = 1) and drops the rest, uniq mode drops
    // every copy (a heavy key occurs more than once: no uniq row); the chain's
    // dropped copies go to hv_drop[hv_idx[j * HV_BSLOTS + slot]] when it ends
    const uint64_t *hv_tab;
    const uint32_t *hv_idx;
    uint64_t *hv_drop;
    uint32_t hv_q, hv_keep;
};

// heavy keys of a key round (kman_dround_finish): found by sampling the
// received items, counted apart in pass 1 so that a satellite or repeat-family
// k-mer with 10^5 copies does not overflow its regions (and send the key range
// through the partial redo)
constexpr uint32_t HV_BSLOTS = 1024, HV_BMAX = 256, HV_MAX = 1u << 16;
constexpr uint64_t HV_EMPTY = ~0ull;
constexpr uint32_t HV_FBITS = 1u << 16;
__host__ __device__ inline uint32_t hv_fbit(uint64_t rest) { return ((uint32_t)rest * 0x85EBCA6Bu) >> 16; }
__host__ __device__ inline uint32_t hv_slot(uint64_t rest) {
    return (((uint32_t)rest ^ (uint32_t)(rest >> 29)) * 0x9E3779B1u) >> 22;  // (one 32-bit multiply)
}
// the heavy-key scratch (kman_ctx::d_hv): what outlives find_heavy
constexpr size_t HVO_TAB = 0, HVO_IDX = HVO_TAB + 256 * HV_BSLOTS * 8, HVO_KEYS = HVO_IDX + 256 * HV_BSLOTS * 4,
                 HVO_DROP = HVO_KEYS + HV_MAX * 8, HVO_END = HVO_DROP + HV_MAX * 8;

// Persistent 1024-thread blocks (one per CU; 141 KiB of LDS), block-owned
// chains: a block takes a whole chain (bucket b, part h: the h-th of H runs of
// the bucket's tiles of PT_NT * PT_SI items) and walks its tiles in order, carrying each
// digit's running count in LDS, so no tile ever waits on another block (no
// look-back, no status words).  Per tile:
//   * loads: logical item -> (segment, offset) by ballots over the lanes'
//     segment prefixes (the 64 items of a wave row are consecutive, so their
//     segment is the row start's, past the rare boundaries inside the row):
//     no LDS and no dependent chain, so the loads issue back to back; the
//     next tile's loads are issued behind this tile's stores;
//   * rank by one block-wide LDS atomic per item (the order of equal digits
//     inside a tile is then not stable, which the finish does not need -- it
//     sorts every remaining key bit and compares keys only), LDS scatter;
//   * write combining: each digit's last partial 128-byte line (< 16 items)
//     stays in LDS until a later tile completes it, so only whole lines leave
//     the CU, each written within one tile's store phase (64 KiB of LDS).
// (512-thread blocks, two per CU, with 64-byte write-combining lines --
// 32 KiB each -- measured slower: 4.32 vs 3.48 ms)
// TI / TO: the items read / written, 8 bytes or 4.  Count items whose key
// bits below this pass's digit fit 32 bits (no window index, no tag: k <= 24
// after pass 0 + 1's 17 bits) are written as 4 bytes -- the digit and the
// bits above it are implied by the sub-region -- so the next pass and the
// finish read half the bytes.
// NT_ / RB: 1024 threads and digits up to 9 bits (141 KiB of LDS, one block
// per CU), or 512 threads and up to 8 bits (4096-item tiles and 256 digits'
// lines, ~69 KiB: two blocks per CU, so one block's loads, rank and scatter
// run while the other's stores stream)
// LN (kman_groups' 8-byte items on the 1024-thread instance): no staged tile
// and 256-byte lines.  The tile's items stay in registers; an item's rank and
// its digit's running count give its position p in the digit's output stream,
// and it goes straight to its line slot in LDS.  The 128 KiB of lines are 512
// lines of 32 items, 2^(9 - bits) of them per digit as a ring over the digit's
// stream (one line per digit at 9 bits); a line leaves the CU only when whole,
// as 16 lanes x 16 bytes, so a store phase writes aligned 256-byte runs only.
// A digit that gets more than its ring holds in one tile is placed in
// block-uniform rounds (place, barrier, store the whole lines, barrier): their
// number comes from the tile's largest per-digit line count -- two placements
// and one store phase on uniform data at any digit width.  Needs C1 a multiple
// of 32 and a 256-byte aligned output (launch_pass_as checks both).
constexpr int PT_NT = 1024, PT_SI = 8;
template <typename TI, typename TO, int NT_ = PT_NT, int RB = R1, bool LN = false, bool HV = false, bool ZB = false>
__global__ __launch_bounds__(NT_, 4) void rg_pass(PassArgs pa, uint32_t *__restrict__ counter,
                                                 uint32_t *__restrict__ err, uint64_t *__restrict__ stp) {
    constexpr int NT = NT_, SI = HV ? PT_SI - 1 : PT_SI, TILE = NT * SI, NWAVE = NT / 64;  // (HV: 7 items, no spills)
    static_assert(!LN || (!HV && !ZB && sizeof(TI) == 8 && sizeof(TO) == 8 && NT == 1024 && RB == 512),
                  "lines of 32 items: the 8-byte, 1024-thread, 512-digit instance");
    // items per write-combining line (128 bytes)
    constexpr uint32_t WLB = sizeof(TO) == 8 ? 4 : 5, WL = 1u << WLB, WM = WL - 1;
    static_assert(NT >= RB && NT / WL <= RB, "a thread per digit");
    __shared__ __attribute__((aligned(16))) TI skeys[LN ? 1 : TILE];
    __shared__ __attribute__((aligned(16))) uint64_t wcb_[LN ? RB * 32 : RB * 16];  // 128 bytes per digit (LN: 256)
    TO(*const wcb)[WL] = reinterpret_cast<TO(*)[WL]>(wcb_);  // the pending items of digit d at wcb[d][pos % WL]
    // pending items leave 16 lanes per digit (one line per quarter wave), EPL
    // items per lane: a 4-byte item's lane stores two as one 8-byte store
    // (its slot j is even and lines are 128-byte aligned)
    constexpr uint32_t EPL = WL / 16;
    auto put_pending = [](TO *dst, const TO *src, bool both) {
        if constexpr (EPL == 2) {
            if (both) {
                *reinterpret_cast<uint2 *>(dst) = *reinterpret_cast<const uint2 *>(src);
                return;
            }
        }
        *dst = *src;
    };
    // per digit for the store loop: qpar[d] = (q bound of the whole-line
    // items << 32) | the output index of tile item 0 relative to the chain's
    // first sub-region (digit d's sub-region is d * gsub * H after it, and
    // C1 is a multiple of 16, so the low 4 bits are the line slot)
    __shared__ uint64_t qpar[LN ? 1 : RB];
    __shared__ uint32_t thist[RB];
    __shared__ uint32_t lstart[LN ? 1 : RB];
    __shared__ uint32_t s_nl;  // LN: the most lines any digit completes in this tile
    __shared__ uint32_t run[RB];  // the chain's running count per digit
    __shared__ uint32_t lds_scan[NWAVE];
    __shared__ uint32_t s_items;
    __shared__ uint32_t lds_tile;
    // HV: the chain's copies of each heavy key (by table slot)
    __shared__ uint64_t htab[HV ? HV_BSLOTS : 1];
    __shared__ uint32_t hcnt[HV ? HV_BSLOTS : 1];
    // a 2^16-bit filter of the table's keys: most items test one bit
    __shared__ uint32_t hbits[HV ? HV_FBITS / 32 : 1];
    const uint32_t shift = pa.shift, bits = pa.bits, nsg = pa.nsg, H = pa.H;
    const uint64_t C1 = pa.C1;
    const int lane = lane_id();
    const int w = threadIdx.x >> 6;
    const uint32_t radix = 1u << bits, dmask = radix - 1;
    const uint32_t nchain = pa.nbk * H;

    for (;;) {
        const uint32_t ch = (uint32_t)grab_tile(counter, &lds_tile);
        if (ch >= nchain) break;
        const uint32_t b = ch / H, h = ch % H;
        // every wave: the bucket's segment prefixes (lane s: items before
        // segment s; segments >= nsg empty) and bases, in registers
        uint32_t spre_l = 0;
        uint64_t sbase_l = 0;
        {
            const uint32_t sgl = (uint32_t)lane;
            const uint64_t gi = (uint64_t)b * nsg + sgl;
            uint32_t c = sgl < nsg ? pa.seg_cnt[pa.cnt_sb ? (uint64_t)sgl * pa.nbk + b : gi] : 0u;
            if (!pa.seg_base && c > pa.stride) c = (uint32_t)pa.stride;  // (an overflowed atomic cursor)
            const uint32_t inc = wave_inclusive_scan(c, SumU32());
            spre_l = inc - c;
            sbase_l = sgl < nsg ? (pa.seg_base ? pa.seg_base[gi] : gi * pa.stride) : 0ull;
            if (threadIdx.x == 63) s_items = inc;
        }
        if (threadIdx.x < RB) run[threadIdx.x] = 0;
        if constexpr (HV) {
            for (uint32_t s = threadIdx.x; s < HV_BSLOTS; s += NT) {
                htab[s] = pa.hv_tab[(uint64_t)(b / pa.gsub) * HV_BSLOTS + s];
                hcnt[s] = 0;
            }
            for (uint32_t s = threadIdx.x; s < HV_FBITS / 32; s += NT) hbits[s] = 0;
        }
        __syncthreads();
        if constexpr (HV) {
            for (uint32_t s = threadIdx.x; s < HV_BSLOTS; s += NT) {
                const uint64_t t = htab[s];
                if (t != HV_EMPTY) {
                    const uint32_t bt = hv_fbit(t);
                    atomicOr(&hbits[bt >> 5], 1u << (bt & 31));
                }
            }
            __syncthreads();
        }
        const uint32_t items = s_items;
        const uint32_t tiles = (items + TILE - 1) / TILE;
        const uint32_t per = (tiles + H - 1) / H;
        const uint32_t ra = h * per, rb = ra + per < tiles ? ra + per : tiles;
        // output sub-region of digit d
        const uint64_t reg0 = (uint64_t)(b / pa.gsub) << bits, rsub = b % pa.gsub;
#define SUBREG(d) (((reg0 | (d)) * pa.gsub + rsub) * H + h)
        // digit d's sub-region is d * dstride items after digit 0's
        TO *const obase0 = static_cast<TO *>(pa.out) + SUBREG(0u) * C1;
        const uint32_t dstride = pa.gsub * H * (uint32_t)C1;
        const uint32_t ib = (uint32_t)(w * (SI * 64) + lane);
        TI key[SI];
        uint32_t sgp[(SI + 3) / 4];  // the items' segments, 8 bits each (for the tag)
        auto rl64 = [](uint64_t v, int l) -> uint64_t {
            return ((uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)(v >> 32), l) << 32) |
                   (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, l);
        };
        auto load_tile = [&](uint32_t rt) {
            const uint32_t tt0 = rt * TILE;
            const uint32_t nn = items - tt0 < (uint32_t)TILE ? items - tt0 : (uint32_t)TILE;
#pragma unroll
            for (int i = 0; i < (SI + 3) / 4; i++) sgp[i] = 0;
            // a wave's rows are consecutive items: the segment of its first
            // row, its base and where the next segment starts, once per tile
            // (wave-uniform, from readlanes); only a row that reaches the
            // next segment takes the per-row ballots
            const uint32_t wfirst = tt0 + (uint32_t)w * (SI * 64);
            uint32_t c_sg, c_po, c_nx;
            uint64_t c_bs;
            auto seg_at = [&](uint32_t li0) {
                const int s0 = __popcll(__ballot(spre_l <= li0) & ~1ull);  // lane 0 (prefix 0) not counted
                c_sg = (uint32_t)s0;
                c_po = (uint32_t)__builtin_amdgcn_readlane((int)spre_l, s0);
                c_bs = rl64(sbase_l, s0);
                c_nx = s0 < 63 ? (uint32_t)__builtin_amdgcn_readlane((int)spre_l, s0 + 1) : ~0u;
            };
            seg_at(wfirst);
#pragma unroll
            for (int i = 0; i < SI; i++) {
                const uint32_t li0 = wfirst + (uint32_t)i * 64;
                const uint32_t li = li0 + (uint32_t)lane;
                uint32_t sg = c_sg, po = c_po;
                uint64_t bs = c_bs;
                if (li0 + 63 >= c_nx) {  // (wave-uniform, rare: the row reaches the next segment)
                    const int sg0 = __popcll(__ballot(spre_l <= li0) & ~1ull);
                    sg = (uint32_t)sg0;
                    bs = rl64(sbase_l, sg0);
                    po = (uint32_t)__builtin_amdgcn_readlane((int)spre_l, sg0);
                    uint64_t inrow = __ballot(spre_l > li0 && spre_l <= li0 + 63);
                    while (inrow) {  // (wave-uniform)
                        const int s2 = __ffsll((unsigned long long)inrow) - 1;
                        inrow &= inrow - 1;
                        const uint32_t p2 = (uint32_t)__builtin_amdgcn_readlane((int)spre_l, s2);
                        if (li >= p2) {
                            sg = (uint32_t)s2;
                            po = p2;
                            bs = rl64(sbase_l, s2);
                        }
                    }
                    seg_at(li0 + 64);
                }
                sgp[i >> 2] |= sg << (8 * (i & 3));
                // (kept as TI: a 4-byte load zero-extended in the branch
                // was waited for inside it, one load at a time)
                key[i] = ib + i * 64 < nn ? static_cast<const TI *>(pa.in)[bs + (li - po)] : (TI)0;
            }
        };
        if (ra < rb) load_tile(ra);
        for (uint32_t r = ra; r < rb; r++) {
            // (double-buffered counts, so that neither this clear nor the
            // update below needs its barrier: no faster, 3.50 vs 3.41-3.50 ms)
            if (threadIdx.x < RB) thist[threadIdx.x] = 0;
            if (LN && threadIdx.x == 0) s_nl = 0;
            __syncthreads();
            const uint32_t t0 = r * TILE;
            const uint32_t n = items - t0 < (uint32_t)TILE ? items - t0 : (uint32_t)TILE;
            RSTAMP(r, 0);
            uint32_t rank[SI];
            if (pa.tag) {
                // (a separate loop, so the loads above are not serialised on it)
                const uint64_t tm = ((1ull << pa.tag_bits) - 1) << pa.tag_shift;
#pragma unroll
                for (int i = 0; i < SI; i++) {
                    const uint32_t sg = (sgp[i >> 2] >> (8 * (i & 3))) & 0xffu;
                    key[i] = (TI)((key[i] & ~tm) | ((uint64_t)(sg / pa.tag_div) << pa.tag_shift));
                }
            }
#define PDIGIT(x) ((uint32_t)((x) >> shift) & dmask)
            // the items that stay (bit i): all but dropped heavy copies
            uint32_t vm = 0;
#pragma unroll
            for (int i = 0; i < SI; i++) vm |= (ib + i * 64 < n ? 1u : 0u) << i;
            if constexpr (HV) {
                // the filter over every item; then each lane probes only its
                // candidates, one per trip (the trips: the most candidates
                // any lane has, mostly 1 -- not one probe path per item)
                uint32_t cm = 0;
#pragma unroll
                for (int i = 0; i < SI; i++) {
                    const uint32_t bt = hv_fbit((uint64_t)key[i] >> pa.hv_q);
                    cm |= (((vm >> i) & (hbits[bt >> 5] >> (bt & 31))) & 1u) << i;
                }
                while (__builtin_amdgcn_read_exec() & __ballot(cm != 0)) {
                    if (cm) {
                        const int i = __ffs(cm) - 1;
                        cm &= cm - 1;
                        uint64_t kk = key[0];
#pragma unroll
                        for (int u = 1; u < SI; u++) kk = i == u ? (uint64_t)key[u] : kk;
                        const uint64_t kr = kk >> pa.hv_q;
                        uint32_t sl = hv_slot(kr);
                        uint64_t t = htab[sl];
                        while (t != kr && t != HV_EMPTY) {  // (<= 1/4 full: short)
                            sl = (sl + 1) & (HV_BSLOTS - 1);
                            t = htab[sl];
                        }
                        if (t == kr) {
                            const uint32_t old = atomicAdd(&hcnt[sl], 1u);
                            if (!(pa.hv_keep && old == 0)) vm &= ~(1u << i);
                        }
                    }
                }
            }
            if constexpr (ZB) {
                // (a 0-bit pass, pass 1b merging the sources' sub-regions: every
                // item to digit 0 in tile order -- no same-address atomics)
#pragma unroll
                for (int i = 0; i < SI; i++) rank[i] = ib + i * 64;
                if (threadIdx.x == 0) thist[0] = n;
            } else {
#pragma unroll
                for (int i = 0; i < SI; i++) rank[i] = (vm >> i) & 1u ? atomicAdd(&thist[PDIGIT(key[i])], 1u) : 0u;
            }
            __syncthreads();
            if constexpr (LN) {
                // digit d's ring: its 2^lb lines, RING items; stream line g
                // (items [32 g, 32 g + 32) of d's sub-region) sits in line
                // (d << lb) | (g & lm); the first line not yet stored is run[d] >> 5
                // (line1, a test setting: one line per digit at any width)
                const uint32_t lb = pa.line1 ? 0u : 9u - bits, lm = (1u << lb) - 1, RING = 32u << lb;
                if (threadIdx.x < RB) {
                    struct MaxU32 {
                        KMAN_DEV uint32_t operator()(uint32_t a, uint32_t b) const { return a > b ? a : b; }
                    };
                    const uint32_t rn = run[threadIdx.x];
                    const uint32_t nl = ((rn + thist[threadIdx.x]) >> 5) - (rn >> 5);
                    const uint32_t m = wave_inclusive_scan(nl, MaxU32(), 0u);
                    if (lane == 63 && m) atomicMax(&s_nl, m);
                }
                // rank[i] <- the item's placement round << 14 | its ring slot
#pragma unroll
                for (int i = 0; i < SI; i++) {
                    const uint32_t rn = run[PDIGIT(key[i])], p = rn + rank[i];
                    rank[i] = ((((p >> 5) - (rn >> 5)) >> lb) << 14) | (p & (RING - 1));
                }
                auto place = [&](uint32_t round) {
#pragma unroll
                    for (int i = 0; i < SI; i++)
                        if (((vm >> i) & 1u) && (rank[i] >> 14) == round)
                            wcb_[PDIGIT(key[i]) * RING + (rank[i] & 0x3fffu)] = key[i];
                };
                place(0);
                __syncthreads();
                RSTAMP(r, 1);
                // the tile completes at most mx lines of a digit: nst store
                // phases (a ring's worth of lines each), npl placements
                const uint32_t mx = s_nl, nst = (mx + lm) >> lb, npl = (mx >> lb) + 1;
                for (uint32_t ph = 0; ph < nst; ph++) {
                    // the lines whole after placement ph, 16 lanes x 16 bytes
                    // each (a wave's store covers 4 lines); lines at or past
                    // the capacity stay (C1 is a multiple of 32)
                    // (SB lines' LDS reads back to back, then their stores; all
                    // eight at once spill)
                    constexpr uint32_t SB = 4;
#pragma unroll
                    for (uint32_t i0 = 0; i0 < RB / (NT / 16); i0 += SB) {
                        uint4 v[SB];
                        uint32_t at[SB];
#pragma unroll
                        for (uint32_t it = 0; it < SB; it++) {
                            const uint32_t x = (threadIdx.x >> 4) + (i0 + it) * (NT / 16), d = x >> lb;
                            const uint32_t rn = run[d], g0 = (rn >> 5) + (ph << lb), g = g0 + ((x - g0) & lm);
                            const bool whole = g < ((rn + thist[d]) >> 5) && g * 32u < C1;
                            at[it] = whole ? d * dstride + g * 32u + (threadIdx.x & 15u) * 2u : ~0u;
                            v[it] = *reinterpret_cast<const uint4 *>(&wcb_[x * 32u + (threadIdx.x & 15u) * 2u]);
                        }
                        // (keeps the reads here: sunk into the branches below,
                        // each store waits for its own read)
#pragma unroll
                        for (uint32_t it = 0; it < SB; it++)
                            asm volatile("" : "+v"(v[it].x), "+v"(v[it].y), "+v"(v[it].z), "+v"(v[it].w));
#pragma unroll
                        for (uint32_t it = 0; it < SB; it++)
                            if (at[it] != ~0u) *reinterpret_cast<uint4 *>(obase0 + at[it]) = v[it];
                    }
                    if (ph + 1 < npl) {
                        __syncthreads();  // those line reads before the next placement
                        place(ph + 1);
                        if (ph + 1 < nst) __syncthreads();
                    }
                }
            } else {
                const uint32_t ls = block_exclusive_scan1<NT>(threadIdx.x < RB ? thist[threadIdx.x] : 0u, SumU32(), 0u,
                                                              lds_scan, (uint32_t *)nullptr);
                if (threadIdx.x < RB) lstart[threadIdx.x] = ls;
                __syncthreads();
#pragma unroll
                for (int i = 0; i < SI; i++)
                    if ((vm >> i) & 1u) skeys[lstart[PDIGIT(key[i])] + rank[i]] = key[i];
                // (HV: the tile's items that stay, packed at the front of skeys)
                const uint32_t nk = HV ? lstart[RB - 1] + thist[RB - 1] : n;
                __syncthreads();
                RSTAMP(r, 1);
                // a digit whose partial line completes in this tile: its pending
                // items go out first, 16 lanes per digit (one line per quarter
                // wave, so a store covers 4 lines)
                // (the LDS reads of this loop and the store loop below issued
                // first, back to back: 3.39 vs 3.31 ms, `r04o_pipe_ab.txt`)
#pragma unroll
                for (uint32_t it = 0; it < RB / (NT / 16); it++) {  // (a constant trip count: unrolled)
                    const uint32_t d = (threadIdx.x >> 4) + it * (NT / 16);
                    const uint32_t j = (threadIdx.x & 15u) * EPL, rn = run[d], p = rn & WM;
                    if (j < p && ((rn + thist[d]) >> WLB) > (rn >> WLB) && rn - p + j < C1)
                        put_pending(obase0 + d * dstride + rn - p + j, &wcb[d][j], j + 1 < p && rn - p + j + 1 < C1);
                }
                if (threadIdx.x < RB) {
                    // item q of digit d goes to position at = q + off; whole lines
                    // end at fe; positions >= C1 are dropped (an overflowing
                    // region raises ERR_REGION, so where its items go is moot)
                    const uint32_t d = threadIdx.x, rn = run[d], off = rn - lstart[d];
                    const int32_t fe = (int32_t)((rn + thist[d]) & ~WM);
                    const int32_t qlim = (fe < (int32_t)C1 ? fe : (int32_t)C1) - (int32_t)off;
                    qpar[d] = ((uint64_t)(uint32_t)qlim << 32) | (d * dstride + off);
                }
                __syncthreads();  // those wcb reads before the leftovers below
                // items of whole lines to HBM, the new partial line to LDS
#pragma unroll
                for (int rr = 0; rr < SI; rr++) {
                    const uint32_t q = threadIdx.x + rr * NT;
                    if (q < nk) {
                        const uint64_t kk = skeys[q];
                        const uint32_t d = PDIGIT(kk);
                        const uint64_t qp = qpar[d];
                        const uint32_t rel = (uint32_t)qp + q;
                        if ((int32_t)q < (int32_t)(qp >> 32)) obase0[rel] = (TO)kk;
                        else wcb[d][rel & WM] = (TO)kk;
                    }
                }
            }
            // the next tile's loads behind the stores (issued before the
            // store phase instead, they overlap it and the pass slows down:
            // 6.2 vs 4.9 ms; issued right after the LDS scatter: 3.80 vs 3.43)
            if (r + 1 < rb) load_tile(r + 1);
            __syncthreads();  // every read of run[] above before its update
            if (threadIdx.x < RB) run[threadIdx.x] += thist[threadIdx.x];
            RSTAMP(r, 2);
#undef PDIGIT
        }
        // the chain's sub-region counts (every digit, also of empty chains)
        __syncthreads();
        // the last partial lines, 16 lanes per digit
        if constexpr (LN) {
            // (the one line of a digit's ring that holds its stream's open line)
            const uint32_t lb = pa.line1 ? 0u : 9u - bits, lm = (1u << lb) - 1;
            // (once per chain; unrolled, its eight addresses are kept, spilled, over the tile loop)
#pragma unroll 1
            for (uint32_t it = 0; it < RB / (NT / 16); it++) {
                const uint32_t x = (threadIdx.x >> 4) + it * (NT / 16), d = x >> lb;
                const uint32_t j = (threadIdx.x & 15u) * 2u, rn = d < radix ? run[d] : 0u, p = rn & 31u;
                if (j < p && ((rn >> 5) & lm) == (x & lm) && rn - p < C1) {
                    TO *const dst = obase0 + d * dstride + rn - p + j;
                    if (j + 1 < p) *reinterpret_cast<uint4 *>(dst) = *reinterpret_cast<const uint4 *>(&wcb_[x * 32u + j]);
                    else *dst = wcb_[x * 32u + j];
                }
            }
        } else {
#pragma unroll
            for (uint32_t it = 0; it < RB / (NT / 16); it++) {
                const uint32_t d = (threadIdx.x >> 4) + it * (NT / 16);
                const uint32_t j = (threadIdx.x & 15u) * EPL, rn = run[d], p = rn & WM;
                if (j < p && rn - p + j < C1)
                    put_pending(static_cast<TO *>(pa.out) + SUBREG(d) * C1 + rn - p + j, &wcb[d][j],
                                j + 1 < p && rn - p + j + 1 < C1);
            }
        }
        if (threadIdx.x < RB) {
            const uint32_t d = threadIdx.x;
            if (run[d] > C1 && d < radix) {
                atomicOr(err, ERR_REGION);
                if (pa.fail) {
                    const uint64_t f0 = (SUBREG(d) / pa.fail_div) << pa.fail_shift;
                    for (uint64_t f = 0; f < (1ull << pa.fail_shift); f++) pa.fail[f0 + f] = 1;
                }
            }
            if (d < radix) pa.cnt1[SUBREG(d)] = run[d] < C1 ? run[d] : (uint32_t)C1;
        }
        if constexpr (HV) {
            // the chain's dropped copies of each heavy key (hcnt is cleared by
            // the next chain only after grab_tile's barriers; the barrier here
            // keeps the index loads below from waiting on the stores above)
            __syncthreads();
            for (uint32_t s = threadIdx.x; s < HV_BSLOTS; s += NT) {
                const uint32_t c = hcnt[s];
                if (c > pa.hv_keep)
                    atomicAdd((unsigned long long *)&pa.hv_drop[pa.hv_idx[(uint64_t)(b / pa.gsub) * HV_BSLOTS + s]],
                              (unsigned long long)(c - pa.hv_keep));
            }
        }
#undef SUBREG
    }
}


// ---------------------------------------------------------------- finish
// One block per region r (regions in key order = grab order): LSD sort of the
// item bits [Q, Q + rest) in LDS (<= 9-bit digits, per-wave counters, stable),
// run-length pass, output compacted through one look-back over the regions.
// COUNT: okeys[j], ovals[j] = group size; UNIQ: keys of groups of one and
// their pos ((window << 1) | strand).
// T = uint32_t (count mode, rest <= 32 bits, no tag): items held as their key
// rest in 4 bytes, half the LDS (three blocks per CU); rows staged in two
// rounds (keys, then counts).
// CHK (uniq): the early row count (below) is checked against the rows the
// sorted keys give -- per thread, the singleton marks against heads & tails
// computed from the keys -- and a disagreement raises ERR_EARLY; CHK = 2 also
// flips one mark of region `hook` (a test of the check itself).
enum { RG_COUNT = 1, RG_UNIQ = 2 };

// waves per SIMD the launch bounds ask for: 8-byte items of a GCAP region
// (40 KiB) and 4-byte items: three blocks per CU; 8-byte items of an FCAP
// region (68 KiB) and the ballot ranks (their registers): two
template <typename T, bool ATOMIC, int CAP>
constexpr int fin_waves() {
    // (4-byte items of a GCAP region, 28 KiB: four blocks per CU in 64
    // VGPRs, 6.46 vs 7.07 ms per 1 G k-mers at three)
    if (sizeof(T) == 4 && CAP <= GCAP) return 8;
    return sizeof(T) == 4 || (ATOMIC && CAP <= GCAP) ? 6 : 4;
}

template <int MODE, typename O, bool ATOMIC, typename T = uint64_t, int CHK = 0, int CAP = FCAP>
__global__ __launch_bounds__(FT, (fin_waves<T, ATOMIC, CAP>())) void rg_finish(
    const uint64_t *__restrict__ in, uint64_t C1, const uint32_t *__restrict__ cnt1, uint32_t Q, uint32_t rest,
    uint32_t rc, uint64_t rbase, uint32_t tag_shift, uint32_t fsub, uint64_t *__restrict__ okeys,
    O *__restrict__ ovals, uint64_t *__restrict__ status, uint32_t *__restrict__ counter, uint32_t epoch,
    uint32_t *__restrict__ err, uint32_t hook, uint64_t *__restrict__ stp, uint32_t nreg,
    uint8_t *__restrict__ freg, uint32_t in4) {
    constexpr int NT = FT, NW_ = NT / 64;
    constexpr int IPT = (CAP + NT - 1) / NT;  // items per thread
    constexpr bool NARROW = sizeof(T) == 4;
    static_assert(!NARROW || MODE == RG_COUNT, "narrow items: count mode");
    // PIPE: the rank atomics and slot reads of a pass issue back to back
    // (8-byte items of an FCAP region, 128 VGPRs).  The 80- and 64-VGPR
    // instances spill so: their ranks stay one round trip at a time and
    // their slot reads go four at a time (count finish 5.34 -> 5.27 ms);
    // the GCAP instance with 3 dwords of spills was no faster on the round
    // path (`r04q_ab.txt`)
    constexpr bool PIPE = ATOMIC && !NARROW && CAP == FCAP;
    static_assert(CHK == 0 || MODE == RG_UNIQ, "the early count is uniq's");
    __shared__ __attribute__((aligned(16))) T s[CAP];
    // per-wave digit counters, u16 pairs; words FWORD + lane: where the
    // lanes without an item add (so every rank atomic is unconditional).
    // TWO (4-byte count items, rest <= 21 bits: the round path's regions):
    // two passes instead of three -- the first by up to 11 bits on ONE
    // block-wide counter array (an LSD sort's first pass need not be stable),
    // the second by up to 10 bits on per-wave counters of 512 words
#ifdef KMAN_NO_TWO
    constexpr bool TWO_OK = false;  // (A/B builds: the three-pass finish everywhere)
#else
    constexpr bool TWO_OK = NARROW;
#endif
    // the two-pass scans cover their counter words with one word pair per
    // thread (first pass: <= 11 bits, 1024 words) and one word per thread
    // (second pass: <= 10 bits, 512 words)
    static_assert(!TWO_OK || (2 * NT >= 1024 && NT >= 512), "the two-pass finish needs >= 512 threads");
    constexpr uint32_t WSTR = TWO_OK ? 512 + 64 : FWORD + 64;
    __shared__ uint32_t wh[NW_][WSTR];
    __shared__ uint32_t lds_scan[NW_], lds_scan2[NW_];
    __shared__ uint32_t s_tile;
    __shared__ uint64_t s_out;

    const int t = threadIdx.x, lane = lane_id(), w = t >> 6;
    const uint64_t rmask = (1ull << rest) - 1;
    const uint32_t pw = (uint32_t)w * (IPT * 64) + (uint32_t)lane;  // wave-striped positions
    // region rr's size m0 (first sub-region) and m (0: emits nothing), and
    // its items into v (wave-striped positions)
    auto region_size = [&](uint32_t rr, uint32_t &m0_) -> uint32_t {
        m0_ = cnt1[(uint64_t)rr * fsub];
        const uint32_t m1_ = fsub > 1 ? cnt1[(uint64_t)rr * fsub + 1] : 0u;
        // freg (the round path): a region flagged by a pass (a sub-region
        // overflowed) or here (more than the LDS holds) emits nothing
        const uint32_t mm = m0_ + m1_;
        if (freg && freg[rr]) return 0u;  // (block-uniform)
        if (mm > (uint32_t)CAP) {
            if (t == 0) {
                atomicOr(err, ERR_REGION);  // (block-uniform) more than the LDS holds
                if (freg) freg[rr] = 1;
            }
            return 0u;
        }
        return mm;
    };
    auto load_items = [&](uint32_t rr, uint32_t m0_, uint32_t mm, T (&v)[IPT]) {
        // (a uniform base and one 32-bit offset per item: few address VGPRs)
        const uint32_t skip = (uint32_t)C1 - m0_;
        if (NARROW && in4) {  // (4-byte count items from the pass: rg_pass<.., uint32_t>)
            const uint32_t *src = reinterpret_cast<const uint32_t *>(in) + (uint64_t)rr * fsub * C1;
#pragma unroll
            for (int i = 0; i < IPT; i++) {
                const uint32_t p = pw + i * 64;
                v[i] = p < mm ? (T)src[p < m0_ ? p : p + skip] : (T)0;
            }
            return;
        }
        const uint64_t *src = in + (uint64_t)rr * fsub * C1;
#pragma unroll
        for (int i = 0; i < IPT; i++) {
            const uint32_t p = pw + i * 64;
            v[i] = p < mm ? (T)src[p < m0_ ? p : p + skip] : (T)0;
        }
    };
    // NARROW (three blocks per CU): wave priority 2 while a region's loads and
    // row stores issue, 0 while it sorts, so the memory phases go ahead of
    // the other blocks' sorting (count finish 5.17 -> 5.08 ms; the uniq
    // instance, two blocks per CU, slows down with it: 5.29 vs 5.21,
    // `r04am_prio_ab.txt`)
    if (NARROW) __builtin_amdgcn_s_setprio(2);
    // one region per block.  (Persistent blocks that load the next region's
    // items into registers while this one is written: 15 vs 6 ms, spilled at
    // three blocks per CU; round 2's at two: 11.1 vs 5.7 ms.)
    if (t == 0) s_tile = atomicAdd(counter, 1u);
    __syncthreads();
    const uint32_t r = __builtin_amdgcn_readfirstlane(s_tile);
    if (r >= nreg) return;
    uint32_t m0;
    const uint32_t m = region_size(r, m0);
    T x[IPT];
    load_items(r, m0, m, x);
    RSTAMP(r, 0);
    if (NARROW) __builtin_amdgcn_s_setprio(0);  // (the sort)
#ifdef KMAN_RG_STAMPS
    __builtin_amdgcn_s_waitcnt(0);  // (diagnostic build: phase 1 = the wait for the region's items)
    if (stp && t == 0) stp[(uint64_t)r * 16 + 15] = m;  // (the region's items, beside its phase stamps)
#endif
    RSTAMP(r, 1);

    // stable LSD passes of <= 9 bits.  Ranks: per-wave u16 counters packed two
    // to a word (a wave ranks <= 64 * IPT items), same-word LDS atomics of one
    // wave return in lane order (probed: ATOMIC), else ballot match-any.
    const bool two = TWO_OK && rest >= 2 && rest <= 21;
    // U32C (8-byte items of an FCAP region: the uniq finish): a block-wide
    // first pass of <= 11 bits, then 8-bit passes on u32 counters (below)
#ifdef KMAN_FIN_U16
    constexpr bool U32C = false;  // (A/B builds: the u16-pair counters, 9-bit passes)
#else
    constexpr bool U32C = PIPE;
#endif
    static_assert(!U32C || (NW_ * (FWORD + 64) >= 2048 + 64 && FWORD + 64 >= 256 + 64), "u32 counters fit wh");
    static_assert(!U32C || NT * IPT <= CAP, "an item past m writes its own position");
    const uint32_t np = two ? 2u : U32C ? (rest <= 11 ? 1u : 1u + (rest - 11 + 7) / 8) : (rest + FBITS - 1) / FBITS;
    const uint32_t bw_two = rest / 2;  // (two: the stable second pass's bits, <= 10)
    // EARLY (uniq): the region's row count is found after the second-to-last
    // pass, when equal keys already share a run of equal low bits (a run of
    // one item almost always), and published then, so the look-back after the
    // last pass finds its predecessors' counts in place instead of waiting
    // for the slowest region in flight (1.0 of 5.8 ms).  A singleton's mark
    // rides in item bit 63 (above the key rest and the pos: the top bit of the
    // pass-1 digit, constant in a region and never read here, so it is
    // overwritten) through the last pass.
    constexpr uint64_t MARK = 1ull << 63;
    // (the round path's items carry the source rank in the 9 bits at
    // tag_shift, read as 8 bits below: bit 63 is free there as well)
    const bool early = MODE == RG_UNIQ && (!tag_shift || tag_shift + 8 <= 63) && np >= 2;
    uint32_t etot = 0;
    uint32_t at = 0;
    uint32_t p0 = 0;
    if constexpr (TWO_OK) {
        if (two) {
            // the first pass, by the low rest - bw_two bits on one block-wide
            // counter array (u16 pairs; the waves' adds interleave, so the
            // pass is not stable, which a first LSD pass need not be)
            uint32_t *const flat = &wh[0][0];
            const uint32_t bw = rest - bw_two, dm = (1u << bw) - 1, nwd = 1u << (bw - 1);
            for (uint32_t q = t; q < nwd; q += NT) flat[q] = 0;
            __syncthreads();
            uint32_t rk[IPT];
#pragma unroll
            for (int i = 0; i < IPT; i++) {
                const uint32_t d = (uint32_t)(x[i] >> Q) & dm, hs = (d & 1u) * 16u;
                rk[i] = pw + i * 64 < m ? (atomicAdd(&flat[d >> 1], 1u << hs) >> hs) & 0xffffu : 0u;
            }
            __syncthreads();
            {
                // thread t: words 2t, 2t+1 (digits 4t .. 4t+3) -> their starts
                // (the scan's barrier orders every word read before the writes)
                const uint32_t c0 = 2 * t < nwd ? flat[2 * t] : 0u, c1 = 2 * t + 1 < nwd ? flat[2 * t + 1] : 0u;
                const uint32_t a0 = c0 & 0xffffu, a1 = c0 >> 16, a2 = c1 & 0xffffu, a3 = c1 >> 16;
                const uint32_t ls =
                    block_exclusive_scan1<NT>(a0 + a1 + a2 + a3, SumU32(), 0u, lds_scan, (uint32_t *)nullptr);
                if (2 * t < nwd) flat[2 * t] = ls | ((ls + a0) << 16);
                if (2 * t + 1 < nwd) flat[2 * t + 1] = (ls + a0 + a1) | ((ls + a0 + a1 + a2) << 16);
            }
            __syncthreads();
#pragma unroll
            for (int i0 = 0; i0 < IPT; i0 += 4) {
                uint32_t sl[4];
#pragma unroll
                for (int i = i0; i < i0 + 4 && i < IPT; i++) {
                    const uint32_t d = (uint32_t)(x[i] >> Q) & dm;
                    sl[i - i0] = ((flat[d >> 1] >> ((d & 1u) * 16u)) & 0xffffu) + rk[i];
                }
#pragma unroll
                for (int i = i0; i < i0 + 4 && i < IPT; i++)
                    if (pw + i * 64 < m) s[sl[i - i0]] = x[i];
                __builtin_amdgcn_sched_barrier(0);
            }
            __syncthreads();
#pragma unroll
            for (int i = 0; i < IPT; i++)
                if (pw + i * 64 < m) x[i] = s[pw + i * 64];
            at = bw;
            p0 = 1;
        }
    }
    // EARLY's marks, after the second-to-last pass (items sorted by their low
    // `at` rest bits, wave-striped in x)
    auto early_marks = [&]() {
            // The items are sorted by their low `at` rest bits, and x holds
            // them wave-striped (item (i, lane) at position pw + i * 64), so a
            // neighbour in position is a neighbouring lane (DPP) or the next /
            // previous row's edge lane (readlane); only the wave's two edges
            // come from LDS.  A key is a singleton iff no item of its run of
            // equal low bits has its whole rest: runs of one or two decide
            // from the neighbours, the rare runs of three or more scan LDS.
            const uint64_t lm = ((1ull << at) - 1) << Q, km = rmask << Q;
            const uint32_t wb = (uint32_t)w * (IPT * 64), we = wb + IPT * 64;
            auto rl64 = [](uint64_t v, int l) -> uint64_t {
                return ((uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)(v >> 32), l) << 32) |
                       (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, l);
            };
            auto eq = [](uint64_t a, uint64_t b, uint64_t mask) { return !((a ^ b) & mask); };
            // the wave's edges: positions wb - 2, wb - 1 and we, we + 1
            const uint64_t eL = wb >= 1 && wb - 1 < m ? (uint64_t)s[wb - 1] : 0;
            const uint64_t eLL = wb >= 2 && wb - 2 < m ? (uint64_t)s[wb - 2] : 0;
            const uint64_t eR = we < m ? (uint64_t)s[we] : 0;
            const uint64_t eRR = we + 1 < m ? (uint64_t)s[we + 1] : 0;
            // LE / FE bit i: item (i, lane) has the low bits / the whole rest
            // of its left neighbour (position - 1)
            uint32_t LE = 0, FE = 0, V = 0;
#pragma unroll
            for (int i = 0; i < IPT; i++) {
                const uint32_t pos = pw + i * 64;
                const uint64_t v = x[i];
                const uint64_t left = wave_shr1(v, i ? rl64(x[i - 1], 63) : eL);
                const bool ok = pos < m && pos > 0;
                const bool le = ok && eq(left, v, lm);
                LE |= (uint32_t)le << i;
                FE |= (uint32_t)(le && eq(left, v, km)) << i;
                V |= (uint32_t)(pos < m) << i;
            }
            // the same of position + 1 (RE, RF), of position - 1 (LL) and of
            // position + 2 (RR): lane shifts, rows carried through lanes 0 / 63
            const uint64_t vlast = rl64(x[IPT - 1], 63);
            const bool eRle = we < m && eq(eR, vlast, lm), eRfe = eRle && eq(eR, vlast, km);
            const bool eRRle = we + 1 < m && eq(eRR, eR, lm);
            const bool eLle = wb >= 2 && wb - 1 < m && eq(eL, eLL, lm);
            const uint32_t top = 1u << (IPT - 1);
            const uint32_t RE = wave_shl1(LE, ((uint32_t)__builtin_amdgcn_readlane((int)LE, 0) >> 1) | (eRle ? top : 0u));
            const uint32_t RF = wave_shl1(FE, ((uint32_t)__builtin_amdgcn_readlane((int)FE, 0) >> 1) | (eRfe ? top : 0u));
            const uint32_t LL = wave_shr1(LE, ((uint32_t)__builtin_amdgcn_readlane((int)LE, 63) << 1) | (eLle ? 1u : 0u));
            const uint32_t RR = wave_shl1(RE, ((uint32_t)__builtin_amdgcn_readlane((int)RE, 0) >> 1) | (eRRle ? top : 0u));
            const uint32_t lng = ((LE & RE) | (LE & LL) | (RE & RR)) & V;  // in a run of three or more
            uint32_t S = V & ~FE & ~RF & ~lng;
            for (uint32_t sl = lng; sl;) {  // (rare: the exact scan over the run in LDS)
                const int i = __ffs(sl) - 1;
                sl &= sl - 1;
                const uint32_t q = pw + (uint32_t)i * 64;
                const uint64_t v = s[q];
                bool single = true;
                for (uint32_t a2 = q; single && a2 > 0;) {
                    const uint64_t u = s[--a2];
                    if (!eq(u, v, lm)) break;
                    if (eq(u, v, km)) single = false;
                }
                for (uint32_t a2 = q + 1; single && a2 < m; a2++) {
                    const uint64_t u = s[a2];
                    if (!eq(u, v, lm)) break;
                    if (eq(u, v, km)) single = false;
                }
                S |= (uint32_t)single << i;
            }
            if (CHK == 2 && r == hook && t == 0) S ^= 1u;  // (the check's own test: one wrong mark)
            // (bit 63 is the top bit of the region's pass-1 digit before it
            // becomes the mark: set or cleared on every item)
#pragma unroll
            for (int i = 0; i < IPT; i++) x[i] = (x[i] & ~(T)MARK) | (((S >> i) & 1u) ? (T)MARK : (T)0);
            (void)block_exclusive_scan1<NT>((uint32_t)__popc(S), SumU32(), 0u, lds_scan2, &etot);
            if (t == 0) publish_agg<0>(status, r, etot, epoch);
    };
    if constexpr (U32C) {
        // the 8-byte-item finish: a first pass by up to 11 bits on ONE
        // block-wide array of u32 counters (unstable, as a first LSD pass may
        // be), then stable passes of <= 8 bits on per-wave u32 counters (256
        // words: no u16 halves to shift in and out); every item's LDS write
        // and read unconditional (an item past m writes its own position,
        // >= m, so no branch per item)
        uint32_t *const flat = &wh[0][0];
        for (uint32_t p = 0; p < np; p++) {
            const bool blk = p == 0;
            const uint32_t bw = blk ? rest - 8 * (np - 1) : 8u;
            const uint32_t sh = Q + at, dm = (1u << bw) - 1;
            at += bw;
            const uint32_t nd = 1u << bw;  // counters of the array
            uint32_t *const wc = blk ? flat : &wh[w][0];
            if (blk) {
                for (uint32_t q = t; q < nd; q += NT) flat[q] = 0;
                __syncthreads();
            } else {
#pragma unroll
                for (int q = 0; q < 256 / 64; q++) wc[lane + 64 * q] = 0;
                __builtin_amdgcn_wave_barrier();
            }
            uint32_t rk[IPT];
#pragma unroll
            for (int i = 0; i < IPT; i++) {
                const bool valid = pw + i * 64 < m;
                const uint32_t d = (uint32_t)(x[i] >> sh) & dm;
                rk[i] = atomicAdd(&wc[valid ? d : nd + lane], 1u);
            }
            __syncthreads();
            if (blk) {
                // thread t: counters [t * cp, (t + 1) * cp), cp = nd / NT (<= 4)
                const uint32_t cp = nd > (uint32_t)NT ? nd / NT : 1u;
                uint32_t c[4] = {0, 0, 0, 0};
                const uint32_t b0 = t * cp;
#pragma unroll
                for (uint32_t q = 0; q < 4; q++)
                    if (q < cp && b0 + q < nd) c[q] = flat[b0 + q];
                uint32_t run = block_exclusive_scan1<NT>(c[0] + c[1] + c[2] + c[3], SumU32(), 0u, lds_scan,
                                                         (uint32_t *)nullptr);
#pragma unroll
                for (uint32_t q = 0; q < 4; q++)
                    if (q < cp && b0 + q < nd) flat[b0 + q] = run, run += c[q];
            } else {
                // thread t < 256: digit t -> its total over the waves, block
                // scan -> digit start, each wave's first slot in place
                uint32_t cw[NW_], tot = 0;
                if (t < 256) {
#pragma unroll
                    for (int ww = 0; ww < NW_; ww++) tot += (cw[ww] = wh[ww][t]);
                }
                uint32_t run = block_exclusive_scan1<NT>(t < 256 ? tot : 0u, SumU32(), 0u, lds_scan,
                                                         (uint32_t *)nullptr);
                if (t < 256) {
#pragma unroll
                    for (int ww = 0; ww < NW_; ww++) wh[ww][t] = run, run += cw[ww];
                }
            }
            __syncthreads();
#pragma unroll
            for (int i = 0; i < IPT; i++) rk[i] += wc[(uint32_t)(x[i] >> sh) & dm];
#ifdef KMAN_FIN_UNCOND
#pragma unroll
            for (int i = 0; i < IPT; i++) {
                const uint32_t pos = pw + i * 64;
                s[pos < m ? rk[i] : pos] = x[i];
            }
#else
            // (only the items: the slot grid past m is 12-14 % of a region's
            // LDS, and writing it unconditionally cost more LDS cycles than
            // the branches: 5.72 vs 5.21 ms, `r06e`)
#pragma unroll
            for (int i = 0; i < IPT; i++)
                if (pw + i * 64 < m) s[rk[i]] = x[i];
#endif
            __syncthreads();
            if (p + 1 < np) {
#pragma unroll
                for (int i = 0; i < IPT; i++)
                    if (pw + i * 64 < m) x[i] = s[pw + i * 64];
            }
            if (early && p + 2 == np) early_marks();
        }
    }
    if constexpr (!U32C)
    for (uint32_t p = p0; p < np; p++) {
        const uint32_t bw = two ? bw_two : (rest - at + (np - p) - 1) / (np - p);
        const uint32_t sh = Q + at, dm = (1u << bw) - 1;
        at += bw;
        // (two: the second pass's per-wave counters, 2^(bw - 1) <= 512 words)
        const uint32_t nwd = two ? 1u << (bw - 1) : (uint32_t)FWORD;
        if (TWO_OK && two) {
            for (uint32_t q = lane; q < nwd; q += 64) wh[w][q] = 0;
        } else {
#pragma unroll
            for (int q = 0; q < FWORD / 64; q++) wh[w][lane + 64 * q] = 0;
        }
        __builtin_amdgcn_wave_barrier();
        uint32_t rk[IPT];
#pragma unroll
        for (int i = 0; i < IPT; i++) {
            const bool valid = pw + i * 64 < m;
            const uint32_t d = (uint32_t)(x[i] >> sh) & dm;
            const uint32_t hs = (d & 1u) * 16u;
            if (PIPE) {
                // (no branch around the atomic: in a branch its return is
                // waited for before the next item's atomic issues, 17 LDS
                // round trips in a row per pass)
                rk[i] = (atomicAdd(&wh[w][valid ? d >> 1 : (uint32_t)FWORD + lane], 1u << hs) >> hs) & 0xffffu;
            } else if (ATOMIC) {
                rk[i] = valid ? (atomicAdd(&wh[w][d >> 1], 1u << hs) >> hs) & 0xffffu : 0u;
            } else {
                uint64_t peers = __ballot(valid);
                for (uint32_t bb = 0; bb < bw; bb++) {
                    const bool set = (d >> bb) & 1u;
                    const uint64_t mm = __ballot(set);
                    peers &= set ? mm : ~mm;
                }
                const uint32_t before = valid ? (wh[w][d >> 1] >> hs) & 0xffffu : 0u;
                rk[i] = before + (uint32_t)__popcll(peers & lanemask_lt());
                __builtin_amdgcn_wave_barrier();
                const int leader = __ffsll((unsigned long long)peers) - 1;
                if (valid && lane == leader) atomicAdd(&wh[w][d >> 1], (uint32_t)__popcll(peers) << hs);
                __builtin_amdgcn_wave_barrier();
            }
        }
        __syncthreads();
        {
            // thread t < words: digits 2t, 2t+1 -> their totals, block scan
            // of the totals -> digit starts, then each wave's first slot per
            // digit (digit start + the earlier waves' counts, < 2^16) in place
            // of its counters, so the scatter reads one word per item
            const uint32_t nw_ = nwd;
            uint32_t tlo = 0, thi = 0, cw[NW_];
            if (t < nw_) {
#pragma unroll
                for (int ww = 0; ww < NW_; ww++) {
                    cw[ww] = wh[ww][t];
                    tlo += cw[ww] & 0xffffu;
                    thi += cw[ww] >> 16;
                }
            }
            const uint32_t ls = block_exclusive_scan1<NT>(tlo + thi, SumU32(), 0u, lds_scan, (uint32_t *)nullptr);
            if (t < nw_) {
                uint32_t plo = ls, phi = ls + tlo;
#pragma unroll
                for (int ww = 0; ww < NW_; ww++) {
                    wh[ww][t] = plo | (phi << 16);
                    plo += cw[ww] & 0xffffu;
                    phi += cw[ww] >> 16;
                }
            }
        }
        __syncthreads();
        if (PIPE) {
            // every item's slot first (unconditional reads, issued back to
            // back; an item past m reads a slot it does not use), then the
            // writes
#pragma unroll
            for (int i = 0; i < IPT; i++) {
                const uint32_t d = (uint32_t)(x[i] >> sh) & dm;
                rk[i] += (wh[w][d >> 1] >> ((d & 1u) * 16u)) & 0xffffu;
            }
#pragma unroll
            for (int i = 0; i < IPT; i++)
                if (pw + i * 64 < m) s[rk[i]] = x[i];
        } else {
#pragma unroll
            for (int i0 = 0; i0 < IPT; i0 += 4) {
                uint32_t sl[4];
#pragma unroll
                for (int i = i0; i < i0 + 4 && i < IPT; i++) {
                    const uint32_t d = (uint32_t)(x[i] >> sh) & dm;
                    sl[i - i0] = ((wh[w][d >> 1] >> ((d & 1u) * 16u)) & 0xffffu) + rk[i];
                }
#pragma unroll
                for (int i = i0; i < i0 + 4 && i < IPT; i++)
                    if (pw + i * 64 < m) s[sl[i - i0]] = x[i];
                __builtin_amdgcn_sched_barrier(0);
            }
        }
        __syncthreads();
        if (p + 1 < np) {
#pragma unroll
            for (int i = 0; i < IPT; i++)
                if (pw + i * 64 < m) x[i] = s[pw + i * 64];
        }
        if (early && p + 2 == np) early_marks();
    }
    if (np == 0) {
#pragma unroll
        for (int i = 0; i < IPT; i++)
            if (pw + i * 64 < m) s[pw + i * 64] = x[i];
        __syncthreads();
    }

    RSTAMP(r, 2);
    // ---- run-length pass (thread t: sorted positions t*IPT ..)
    const uint32_t q0 = (uint32_t)t * IPT;
    uint32_t heads = 0, tails = 0;
#define RKEY(v) (((v) >> Q) & rmask)
    T kv[IPT];
#pragma unroll
    for (int j = 0; j < IPT; j++) kv[j] = q0 + j < m ? s[q0 + j] : 0;
    if (early) {
        // the early count's marks are the rows (heads & tails below)
        uint32_t marks = 0;
#pragma unroll
        for (int j = 0; j < IPT; j++) marks |= (uint32_t)(q0 + j < m && ((uint64_t)kv[j] & MARK)) << j;
        heads = tails = marks;
        if (CHK) {
            // the rows the sorted keys give: a singleton differs from both
            // neighbours in its whole rest
            uint32_t single = 0;
            const uint64_t kl = q0 > 0 && q0 - 1 < m ? RKEY((uint64_t)s[q0 - 1]) : ~0ull;
            const uint64_t kr = q0 + IPT < m ? RKEY((uint64_t)s[q0 + IPT]) : ~0ull;
#pragma unroll
            for (int j = 0; j < IPT; j++) {
                const uint32_t q = q0 + j;
                const uint64_t kq = RKEY((uint64_t)kv[j]);
                const bool h = q == 0 || kq != (j ? RKEY((uint64_t)kv[j - 1]) : kl);
                const bool e = q + 1 == m || kq != (j + 1 < IPT ? RKEY((uint64_t)kv[j + 1]) : kr);
                single |= (uint32_t)(q < m && h && e) << j;
            }
            if (single != marks) atomicOr(err, ERR_EARLY);
        }
    } else {
#pragma unroll
        for (int j = 0; j < IPT; j++) {
            const uint32_t q = q0 + j;
            if (q < m) {
                const uint64_t kq = RKEY(kv[j]);
                const bool h = q == 0 || kq != RKEY(j ? kv[j - 1] : s[q - 1]);
                const bool e = q + 1 == m || kq != RKEY(j + 1 < IPT ? kv[j + 1] : s[q + 1]);
                heads |= (uint32_t)h << j;
                tails |= (uint32_t)e << j;
            }
        }
    }
    uint32_t emit = 0, lh_before = 0;
    if constexpr (MODE == RG_UNIQ) {
        emit = heads & tails;
    } else {
        emit = tails;
        const uint32_t lh = heads ? q0 + (31 - __clz(heads)) + 1 : 0u;
        lh_before = block_exclusive_scan1<NT>(
            lh, [](uint32_t a, uint32_t b) { return a > b ? a : b; }, 0u, lds_scan2, (uint32_t *)nullptr);
    }
    const uint32_t ne = (uint32_t)__popc(emit);
    uint32_t total;
    // (its barrier orders every read of s above before the staging writes below)
    const uint32_t off = block_exclusive_scan1<NT>(ne, SumU32(), 0u, lds_scan, &total);
    if (early && t == 0 && total != etot) atomicOr(err, ERR_EARLY);  // (the published count is not the rows')
    RSTAMP(r, 3);
    if (w == 0) {
        const uint64_t ob = early ? wave_lookback_published<0>(status, r, total, epoch, err)
                                  : wave_lookback<0>(status, r, total, epoch, err);
        if (lane == 0) s_out = ob;
    }
    // the emitted rows compacted in LDS as one word each: the item itself
    // (UNIQ: key rest + pos) or key rest | group size << rest (COUNT); every
    // read of s above came before the scan's barriers.  NARROW: the key
    // rests, then (after they are written) the group sizes
    auto stage = [&](bool sizes) {
        uint32_t o = off, cur = lh_before;  // head position + 1 of the open group
#pragma unroll
        for (int j = 0; j < IPT; j++) {
            const uint32_t q = q0 + j;
            if (MODE != RG_UNIQ && ((heads >> j) & 1u)) cur = q + 1;
            if ((emit >> j) & 1u) {
                if constexpr (NARROW)
                    s[o++] = sizes ? (T)(q + 2 - cur) : kv[j];
                else
                    s[o++] = MODE == RG_UNIQ ? kv[j] : (T)(RKEY(kv[j]) | ((uint64_t)(q + 2 - cur) << rest));
            }
        }
    };
    stage(false);
    __syncthreads();
    RSTAMP(r, 4);
    if (NARROW) __builtin_amdgcn_s_setprio(2);  // (the row stores)
    const uint64_t ob = s_out;
    // the rows leave with non-temporal stores (a stream of GBs that no cache
    // keeps until it is read): 5.52-5.58 vs 5.58-5.62 ms (`r04k_nt_ab.txt`;
    // on the passes' scattered line stores they lose L2's write combining:
    // rg_pass 6.3-8.0 vs 3.5 ms)
    const uint64_t qmask = Q ? ((1ull << Q) - 1) : 0ull;
    // OB rows per trip, their LDS reads first, back to back (rows outside
    // the region's read slot 0 and are not written).  Lane l of a wave
    // writes a global row = l mod 64 (the region's first row shifted by
    // ob % 64), so a wave's store covers whole 128-byte lines: non-temporal
    // stores of part lines are not merged in L2 (finish writes 12.35 GB per
    // launch unaligned, 11.74 aligned, `r04s_ab.txt`; same time)
    const uint32_t mis = (uint32_t)(ob & 63);
    constexpr uint32_t OB = 4;
    auto each_row = [&](auto &&put) {
        for (uint32_t q0 = t; q0 < total + mis; q0 += OB * NT) {
            uint64_t v4[OB];
#pragma unroll
            for (uint32_t u = 0; u < OB; u++) {
                const uint32_t q = q0 + u * NT - mis;
                v4[u] = (uint64_t)s[q < total ? q : 0u];
            }
#pragma unroll
            for (uint32_t u = 0; u < OB; u++) {
                const uint32_t q = q0 + u * NT - mis;
                if (q < total) put(q, v4[u]);
            }
        }
    };
    each_row([&](uint32_t q, uint64_t v) {
        __builtin_nontemporal_store(((uint64_t)(r + rbase) << rest) | RKEY(v), okeys + ob + q);
    });
    if constexpr (NARROW) {
        __syncthreads();  // (every key read before the sizes overwrite them)
        stage(true);
        __syncthreads();
    }
    each_row([&](uint32_t q, uint64_t v) {
        if constexpr (MODE == RG_UNIQ) {
            const uint64_t idx = v & qmask;
            const uint64_t pos = rc ? idx : (idx << 1);
            // N > 1: the source rank (tagged into the item by the pass after
            // the exchange) in bits 56-63, as DistPipeline's payloads
            // (ranks < 256: 8 tag bits, so bit 63 -- the early count's mark -- is not read)
            __builtin_nontemporal_store((O)(tag_shift ? pos | (((v >> tag_shift) & 0xffull) << 56) : pos), ovals + ob + q);
        } else if constexpr (NARROW) {
            __builtin_nontemporal_store((O)v, ovals + ob + q);
        } else {
            __builtin_nontemporal_store((O)(v >> rest), ovals + ob + q);
        }
    });
#undef RKEY
    RSTAMP(r, 5);
}

struct RegionPlan {
    uint32_t K, Q, B2, rest;
    bool rc;
    uint64_t W;          // windows (x2 with rc): bound on the k-mers
    bool canon;          // canonical keys (KMAN_CANONICAL)
    bool mix;            // canonical keys through mix_key (KMAN_MIXED: spectra)
    uint64_t C0, C1;     // region capacities (items)
    uint32_t H;          // pass-1 chains (sub-regions) per bucket
    uint64_t C1h;        // pass-1 sub-region capacity
    uint32_t n_tiles0, seg_tiles, maxt1;
    uint32_t ei;         // windows per thread of pass 0
    uint64_t off_r1, off_c0, off_c1, off_lim, bytes;
};

uint32_t bitlen(uint64_t x) { return x ? 64u - (uint32_t)__builtin_clzll(x) : 0u; }

int make_plan(uint64_t n_bases, uint32_t k, uint32_t flags, int mode, RegionPlan *pl) {
    if (mode != KMAN_FINISH_COUNT && mode != KMAN_FINISH_UNIQ) return KMAN_EINVAL;
    if (k < 2 || k > 32) return KMAN_EINVAL;
    if (getenv("KMAN_NO_REGION")) return KMAN_EFALLBACK;  // (tests: the general path)
    // uniq: k <= 25 (the tile-local window index rides above the key bits in
    // pass 0); count items carry no index: k <= 32
    if ((mode == KMAN_FINISH_UNIQ && k > 25) || n_bases == 0) return KMAN_EFALLBACK;
    RegionPlan p{};
    // canonical: one key per window, min(forward, reverse complement)
    p.canon = flags & KMAN_CANONICAL;
    p.mix = p.canon && (flags & KMAN_MIXED);
    p.rc = (flags & KMAN_RC) && !p.canon;
    p.K = 2 * k;
    p.W = n_bases * (p.rc ? 2 : 1);
    p.Q = mode == KMAN_FINISH_UNIQ ? (bitlen(p.W - 1) ? bitlen(p.W - 1) : 1u) : 0u;
    if (p.K - G1 + p.Q > 64) return KMAN_EFALLBACK;
    // B2: fewest bits with an expected region fill <= FFILL_T (at most 9); up
    // to FFILL_M expected keeps > 10 sd (uniform data) below the capacity
    uint32_t b2 = 1;
    // (17 region bits in all while their fill stays <= FFILL_M: the finish's
    // per-region costs make more, smaller regions slower)
    while (b2 < 9 && (p.W >> (G1 + b2)) > FFILL_T && (G1 + b2 < 17 || (p.W >> (G1 + b2)) > FFILL_M)) b2++;
    if ((p.W >> (G1 + b2)) > FFILL_M) return KMAN_EFALLBACK;
    if (p.K < G1 + b2 + 1) return KMAN_EFALLBACK;
    p.B2 = b2;
    p.rest = p.K - G1 - b2;
    // windows per thread: 16 (8 with -r: two items per window) makes
    // 8192-item tiles, 69 KiB of LDS, two blocks per CU: with the atomic
    // region cursors a tile waits on nothing and the longer digit runs win
    // (3.27 vs 3.35 ms with 12 windows, three blocks per CU; 8, four blocks:
    // 3.83)
    p.ei = p.rc ? 8u : 16u;
    const uint64_t win = (uint64_t)RT * p.ei;
    p.n_tiles0 = (uint32_t)ceil_div(n_bases, win);
    p.seg_tiles = (uint32_t)ceil_div(p.n_tiles0, RS);
    const uint64_t nb0 = 1ull << G1;  // pass-0 buckets
    const uint64_t e0 = p.W / (nb0 * RS);
    p.C0 = ceil_div(e0 + e0 / 2 + 256, 64) * 64;
    if (nb0 * RS * p.C0 >= (1ull << 32)) return KMAN_EFALLBACK;  // (32-bit item indices)
    const uint64_t e1 = p.W >> (G1 + b2);
    uint64_t c1 = ceil_div(e1 + e1 / 2 + 512, 64) * 64;
    // (a multiple of 32 either way, and off_r1 of 512 bytes: pass 1's 256-byte lines)
    static_assert(FCAP % 32 == 0, "a sub-region ends on a 256-byte line");
    p.C1 = c1 < (uint64_t)FCAP ? c1 : (uint64_t)FCAP;
    // pass 1 runs H = 2 block-owned chains per bucket (its first and second
    // half of tiles) into H sub-regions per region that the finish
    // concatenates: 512 chains for the 256 resident blocks
    p.H = 2;
    p.C1h = p.C1;  // either half may hold most of a region (position-skewed repeats)
    p.maxt1 = (uint32_t)ceil_div((uint64_t)ceil_div(RS, p.H) * p.C0, T1);
    const uint64_t nreg = 1ull << (G1 + b2);
    p.off_r1 = nb0 * RS * p.C0 * 8;
    p.off_c0 = p.off_r1 + nreg * p.H * p.C1h * 8;
    p.off_c1 = p.off_c0 + nb0 * RS * 4;
    p.off_lim = p.off_c1 + nreg * p.H * 4;
    p.bytes = p.off_lim + 64;
    *pl = p;
    return KMAN_OK;
}

template <typename TI, typename TO>
void launch_pass_as(kman_ctx *ctx, const PassArgs &pa, uint32_t *counter, uint64_t *stp) {
    if constexpr (sizeof(TI) == 8) {
        if (pa.hv_tab) {  // (pass 1 of a key round with heavy keys: 9 bits, the 1024-thread instance)
            const uint32_t grid = (uint32_t)kman_persistent_grid(ctx, (const void *)rg_pass<TI, TO, PT_NT, R1, false, true>,
                                                                 PT_NT, (uint64_t)pa.nbk * pa.H);
            hipLaunchKernelGGL((rg_pass<TI, TO, PT_NT, R1, false, true>), dim3(grid), dim3(PT_NT), 0, ctx->stream, pa, counter,
                               ctx->d_err, stp);
            return;
        }
    }
    if (pa.bits == 0) {  // (a 0-bit pass: pass 1b merging the sources' sub-regions -- its own instance)
        const uint32_t grid = (uint32_t)kman_persistent_grid(ctx, (const void *)rg_pass<TI, TO, 512, 256, false, false, true>,
                                                             512, (uint64_t)pa.nbk * pa.H);
        hipLaunchKernelGGL((rg_pass<TI, TO, 512, 256, false, false, true>), dim3(grid), dim3(512), 0, ctx->stream, pa, counter,
                           ctx->d_err, stp);
        return;
    }
    // radix <= 256: the 512-thread instance, two blocks per CU (KMAN_PASS_SMALL=0: the 1024-thread one)
    static const bool small_ok = !getenv("KMAN_PASS_SMALL") || strcmp(getenv("KMAN_PASS_SMALL"), "0") != 0;
    if (small_ok && pa.bits <= 8 && !pa.big) {
        const uint32_t grid = (uint32_t)kman_persistent_grid(ctx, (const void *)rg_pass<TI, TO, 512, 256>, 512,
                                                             (uint64_t)pa.nbk * pa.H);
        hipLaunchKernelGGL((rg_pass<TI, TO, 512, 256>), dim3(grid), dim3(512), 0, ctx->stream, pa, counter,
                           ctx->d_err, stp);
        return;
    }
#ifndef KMAN_PASS_TILE  // (-DKMAN_PASS_TILE: the staged-tile body for these items too, for A/B)
    if constexpr (sizeof(TI) == 8 && sizeof(TO) == 8) {
        // whole 256-byte lines: every sub-region starts on one and ends on one
        if (pa.lines && pa.C1 % 32 == 0 && (uintptr_t)pa.out % 256 == 0) {
            const uint32_t grid = (uint32_t)kman_persistent_grid(
                ctx, (const void *)rg_pass<TI, TO, PT_NT, R1, true>, PT_NT, (uint64_t)pa.nbk * pa.H);
            hipLaunchKernelGGL((rg_pass<TI, TO, PT_NT, R1, true>), dim3(grid), dim3(PT_NT), 0,
                               ctx->stream, pa, counter, ctx->d_err, stp);
            return;
        }
    }
#endif
    const uint32_t grid =
        (uint32_t)kman_persistent_grid(ctx, (const void *)rg_pass<TI, TO>, PT_NT, (uint64_t)pa.nbk * pa.H);
    hipLaunchKernelGGL((rg_pass<TI, TO>), dim3(grid), dim3(PT_NT), 0, ctx->stream, pa, counter, ctx->d_err, stp);
}

// in4 / out4: the pass reads / writes 4-byte items (out4 only when every key
// bit below the digit fits 32 bits: pa.shift <= 32, and no tag)
void launch_pass(kman_ctx *ctx, const PassArgs &pa, uint32_t *counter, uint64_t *stp, bool in4 = false,
                 bool out4 = false) {
    if (in4) launch_pass_as<uint32_t, uint32_t>(ctx, pa, counter, stp);
    else if (out4) launch_pass_as<uint64_t, uint32_t>(ctx, pa, counter, stp);
    else launch_pass_as<uint64_t, uint64_t>(ctx, pa, counter, stp);
}

struct FinishArgs {
    const uint64_t *in;
    uint64_t C1;
    const uint32_t *cnt;
    uint32_t Q, rest, rc;
    uint64_t rbase;
    uint32_t tag_shift;
    uint32_t nreg;
    uint32_t fsub = 1;  // sub-regions per region (cnt and in indexed per sub-region)
    uint8_t *freg = nullptr;  // per-region overflow flags (the round path), else null
    int cap = FCAP;  // the finish's region capacity: FCAP (kman_groups) or GCAP / FCAP chosen by the round plan
    bool in4 = false;  // 4-byte items (the pass wrote them narrow: only with the narrow finish, narrow_ok)
};

template <int MODE, typename O, int CAP, bool ATOMIC, typename T = uint64_t, int CHK = 0>
void launch_finish_as(kman_ctx *ctx, const FinishArgs &f, uint64_t *okeys, void *ovals, uint32_t epoch,
                      uint32_t *counter, uint32_t hook, uint64_t *stp) {
    hipLaunchKernelGGL((rg_finish<MODE, O, ATOMIC, T, CHK, CAP>), dim3(f.nreg), dim3(FT), 0, ctx->stream, f.in, f.C1,
                       f.cnt, f.Q, f.rest, f.rc, f.rbase, f.tag_shift, f.fsub, okeys, (O *)ovals, ctx->d_status,
                       counter, epoch, ctx->d_err, hook, stp, f.nreg, f.freg, (uint32_t)f.in4);
}

// The early-count check of the uniq finish (rg_finish CHK): KMAN_RG_CHECK=1
// (or "hook=<region>": also one wrong mark in that region, the check's own
// GPU test) selects the checked kernel; 0 / unset, the plain one.
struct EarlyCheck {
    int chk;
    uint32_t hook;
};
EarlyCheck early_check() {
    const char *e = getenv("KMAN_RG_CHECK");
    if (!e || !*e || !strcmp(e, "0")) return {0, ~0u};
    if (!strncmp(e, "hook=", 5)) return {2, (uint32_t)strtoul(e + 5, nullptr, 10)};
    return {1, ~0u};
}

// one block per region; count rows whose key rest fits 32 bits hold 4-byte
// items in LDS (three blocks per CU: count finish 5.95 -> 5.68 ms, config-4
// shard 84.7 -> 78.3 ms).  Without the probed lane-ordered LDS atomics the
// ranks are ballots (8-byte items: the ballot ranks overflow the 80 VGPRs of
// three blocks per CU -- 2.5 KB of spills per lane -- so no narrow variant).
// the narrow (4-byte) count finish's condition -- also when the pass before
// it writes 4-byte items (FinishArgs::in4)
bool narrow_ok(const kman_ctx *ctx, int mode, uint32_t Q, uint32_t rest, uint32_t tag_shift) {
    return mode == KMAN_FINISH_COUNT && ctx->lds_atomic_ordered && rest <= 32 && Q == 0 && tag_shift == 0;
}

template <int MODE, typename O, int CAP>
void launch_finish(kman_ctx *ctx, const FinishArgs &f, uint64_t *okeys, void *ovals, uint32_t epoch,
                   uint32_t *counter, uint64_t *stp) {
    if constexpr (MODE == RG_COUNT) {
        if (narrow_ok(ctx, KMAN_FINISH_COUNT, f.Q, f.rest, f.tag_shift)) {
            launch_finish_as<MODE, O, CAP, true, uint32_t>(ctx, f, okeys, ovals, epoch, counter, ~0u, stp);
            return;
        }
    }
    if (!ctx->lds_atomic_ordered) {
        launch_finish_as<MODE, O, CAP, false>(ctx, f, okeys, ovals, epoch, counter, ~0u, stp);
        return;
    }
    if constexpr (MODE == RG_UNIQ) {
        const EarlyCheck ck = early_check();
        if (ck.chk == 1) {
            launch_finish_as<MODE, O, CAP, true, uint64_t, 1>(ctx, f, okeys, ovals, epoch, counter, ~0u, stp);
            return;
        }
        if (ck.chk == 2) {
            launch_finish_as<MODE, O, CAP, true, uint64_t, 2>(ctx, f, okeys, ovals, epoch, counter, ck.hook, stp);
            return;
        }
    }
    launch_finish_as<MODE, O, CAP, true>(ctx, f, okeys, ovals, epoch, counter, ~0u, stp);
}

template <int CAP>
void launch_finish_cap(kman_ctx *ctx, const FinishArgs &f, int mode, uint64_t *okeys, void *ovals,
                       uint32_t oval_bytes, uint32_t epoch, uint32_t *counter, uint64_t *stp) {
    if (mode == KMAN_FINISH_UNIQ) {
        if (oval_bytes == 4) launch_finish<RG_UNIQ, uint32_t, CAP>(ctx, f, okeys, ovals, epoch, counter, stp);
        else launch_finish<RG_UNIQ, uint64_t, CAP>(ctx, f, okeys, ovals, epoch, counter, stp);
    } else {
        if (oval_bytes == 4) launch_finish<RG_COUNT, uint32_t, CAP>(ctx, f, okeys, ovals, epoch, counter, stp);
        else launch_finish<RG_COUNT, uint64_t, CAP>(ctx, f, okeys, ovals, epoch, counter, stp);
    }
}

int run_finish(kman_ctx *ctx, const FinishArgs &f, int mode, uint64_t *okeys, void *ovals, uint32_t oval_bytes,
               uint64_t *stp) {
    uint32_t epoch, *counter;
    KMAN_TRY(kman_lookback_begin(ctx, f.nreg + 1, &epoch, &counter));
    KTimer kt_(ctx, "region_finish");
    if (f.cap == GCAP) launch_finish_cap<GCAP>(ctx, f, mode, okeys, ovals, oval_bytes, epoch, counter, stp);
    else launch_finish_cap<FCAP>(ctx, f, mode, okeys, ovals, oval_bytes, epoch, counter, stp);
    HIP_TRY(ctx, hipGetLastError());
    return KMAN_OK;
}

// The error word of the region kernels: ERR_REGION alone is not a fault (a
// region that would overflow: the caller redoes the input, or its key ranges,
// by another path); any other bit is, and each has its own message.
int region_fault(kman_ctx *ctx, uint32_t e, const char *what) {
    const uint32_t f = e & ~ERR_REGION;
    if (f & ERR_EARLY)
        return kman_fail(ctx, KMAN_EHIP,
                         "%s: a region's early row count disagreed with the rows its sorted keys give (device "
                         "check, error word %u)", what, e);
    return kman_fail(ctx, KMAN_ETIMEOUT, "%s: device look-back wait exceeded its bound (error word %u)", what, e);
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

void launch_extract_any(kman_ctx *ctx, const RegionPlan &p, const uint8_t *codes, uint64_t n_bases, uint32_t k,
                        uint64_t *r0, uint32_t *c0, uint32_t epoch, uint32_t *counter, uint64_t *stp,
                        uint32_t n_launch = 0) {
    if (p.canon && p.mix) launch_extract<16, false, 2>(ctx, p, codes, n_bases, k, r0, c0, epoch, counter, stp, n_launch);
    else if (p.canon) launch_extract<16, false, 1>(ctx, p, codes, n_bases, k, r0, c0, epoch, counter, stp, n_launch);
    else if (p.rc) launch_extract<8, true>(ctx, p, codes, n_bases, k, r0, c0, epoch, counter, stp, n_launch);
    else launch_extract<16, false>(ctx, p, codes, n_bases, k, r0, c0, epoch, counter, stp, n_launch);
}

// mean phase durations (us) per kernel from the stamp rows; frees the buffers
// the round finish's regions (KMAN_RG_STAMPS diagnostic build): mean phases,
// the spread of per-region times and of the look-back wait, by region size
int report_finish_stamps(kman_ctx *ctx, uint64_t *st, uint64_t nreg) {
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    std::vector<uint64_t> h(nreg * 16);
    HIP_TRY(ctx, hipMemcpy(h.data(), st, h.size() * 8, hipMemcpyDeviceToHost));
    HIP_TRY(ctx, hipFree(st));
    std::vector<double> tot, wait;
    double ph[7] = {0}, sz_t[4] = {0};
    uint64_t n = 0, sz_n[4] = {0}, t0 = ~0ull, t1 = 0;
    for (uint64_t r = 0; r < nreg; r++) {
        const uint64_t *x = &h[r * 16];
        if (!x[0] || !x[5]) continue;
        t0 = x[0] < t0 ? x[0] : t0;
        t1 = x[5] > t1 ? x[5] : t1;
        for (int i = 1; i < 6; i++) ph[i] += (double)(x[i] - x[i - 1]) / 100.0;
        tot.push_back((double)(x[5] - x[0]) / 100.0);
        wait.push_back((double)(x[4] - x[3]) / 100.0);
        const int b = x[15] < 2048 ? 0 : x[15] < 4096 ? 1 : x[15] < 6144 ? 2 : 3;
        sz_t[b] += tot.back();
        sz_n[b]++;
        n++;
    }
    if (!n) return KMAN_OK;
    auto pct = [](std::vector<double> v, double q) {
        std::sort(v.begin(), v.end());
        return v[(size_t)(q * (double)(v.size() - 1))];
    };
    fprintf(stderr, "stamps round finish: regions %llu span %.1f us  mean us/region %.2f  phases:",
            (unsigned long long)n, (double)(t1 - t0) / 100.0, pct(tot, 0.5));
    for (int i = 1; i < 6; i++) fprintf(stderr, " %d:%.2f", i, ph[i] / (double)n);
    fprintf(stderr, "\n  total p50 %.2f p90 %.2f p99 %.2f max %.2f | look-back wait p50 %.2f p90 %.2f p99 %.2f max %.2f\n",
            pct(tot, 0.5), pct(tot, 0.9), pct(tot, 0.99), pct(tot, 1.0), pct(wait, 0.5), pct(wait, 0.9),
            pct(wait, 0.99), pct(wait, 1.0));
    fprintf(stderr, "  mean us by items <2K %.2f (%llu) <4K %.2f (%llu) <6K %.2f (%llu) >=6K %.2f (%llu)\n",
            sz_n[0] ? sz_t[0] / sz_n[0] : 0.0, (unsigned long long)sz_n[0], sz_n[1] ? sz_t[1] / sz_n[1] : 0.0,
            (unsigned long long)sz_n[1], sz_n[2] ? sz_t[2] / sz_n[2] : 0.0, (unsigned long long)sz_n[2],
            sz_n[3] ? sz_t[3] / sz_n[3] : 0.0, (unsigned long long)sz_n[3]);
    return KMAN_OK;
}

int report_stamps(kman_ctx *ctx, uint64_t **st, const uint64_t *rows) {
    static const char *names[3] = {"rg_extract", "rg_pass", "rg_finish"};
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    for (int q = 0; q < 3; q++) {
        std::vector<uint64_t> h(rows[q] * 16);
        HIP_TRY(ctx, hipMemcpy(h.data(), st[q], h.size() * 8, hipMemcpyDeviceToHost));
        HIP_TRY(ctx, hipFree(st[q]));
        double sum[16] = {0}, tot = 0;
        uint64_t n[16] = {0}, nt = 0;
        for (uint64_t r = 0; r < rows[q]; r++) {
            const uint64_t *x = &h[r * 16];
            int last = 0;
            for (int i = 1; i < 15; i++)
                if (x[i] && x[i - 1]) {
                    sum[i] += (double)(x[i] - x[i - 1]) / 100.0;
                    n[i]++;
                    last = i;
                }
            if (x[0] && last) {
                tot += (double)(x[last] - x[0]) / 100.0;
                nt++;
            }
        }
        fprintf(stderr, "stamps %-10s tiles %8llu  mean us/tile %.2f  phases:", names[q], (unsigned long long)nt,
                nt ? tot / nt : 0.0);
        for (int i = 1; i < 15; i++)
            if (n[i]) fprintf(stderr, " %d:%.2f", i, sum[i] / n[i]);
        fprintf(stderr, "\n");
    }
    return KMAN_OK;
}

}  // namespace

extern "C" int kman_groups_plan(uint64_t n_bases, uint32_t k, uint32_t flags, int mode, uint64_t *work_bytes) {
    if (!work_bytes) return KMAN_EINVAL;
    RegionPlan p;
    const int rc = make_plan(n_bases, k, flags, mode, &p);
    *work_bytes = rc == KMAN_OK ? p.bytes : 0;
    return rc;
}

namespace {

// one kman_groups call: the plan and the work-area carve-up
struct GroupsCall {
    RegionPlan p;
    uint64_t *r0, *r1;
    uint32_t *c0, *c1;
    uint32_t nreg;
};

int groups_setup(kman_ctx *ctx, uint64_t n_bases, uint32_t k, uint32_t flags, int mode, void *d_work,
                 uint64_t work_bytes, GroupsCall *g) {
    RegionPlan &p = g->p;
    const int prc = make_plan(n_bases, k, flags, mode, &p);
    if (prc == KMAN_EINVAL) return kman_fail(ctx, KMAN_EINVAL, "kman_groups: bad mode or k");
    if (prc != KMAN_OK) return prc;
    if (!d_work) return kman_fail(ctx, KMAN_EINVAL, "null buffer");
    if (work_bytes < p.bytes)
        return kman_fail(ctx, KMAN_ECAP, "work area %llu < %llu bytes", (unsigned long long)work_bytes,
                         (unsigned long long)p.bytes);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    g->r0 = (uint64_t *)d_work;
    g->r1 = (uint64_t *)((char *)d_work + p.off_r1);
    g->c0 = (uint32_t *)((char *)d_work + p.off_c0);
    g->c1 = (uint32_t *)((char *)d_work + p.off_c1);
    g->nreg = 1u << (G1 + p.B2);
    return KMAN_OK;
}

int groups_outputs_ok(kman_ctx *ctx, const GroupsCall &g, int mode, const void *d_okeys, const void *d_ovals,
                      uint32_t oval_bytes, uint64_t n_bases) {
    if (!d_okeys || !d_ovals) return kman_fail(ctx, KMAN_EINVAL, "null buffer");
    if (oval_bytes != 4 && oval_bytes != 8) return kman_fail(ctx, KMAN_EINVAL, "oval_bytes must be 4 or 8");
    if (oval_bytes == 4 && mode == KMAN_FINISH_UNIQ && (g.p.rc ? g.p.W : 2 * g.p.W) - 1 > 0xffffffffull)
        return kman_fail(ctx, KMAN_EINVAL, "u32 pos cannot address %llu bases", (unsigned long long)n_bases);
    return KMAN_OK;
}

// pass 1 (per bucket, by the next B2 bits), the finish (one block per
// region) and the results: output count (the last region's inclusive),
// region-0 counts (k-mers), error word
int groups_tail(kman_ctx *ctx, const GroupsCall &g, int mode, uint64_t *d_okeys, void *d_ovals, uint32_t oval_bytes,
                uint64_t **stamps, const uint64_t *stamp_rows, uint64_t *n_kmers, uint64_t *n_out) {
    const RegionPlan &p = g.p;
    uint32_t epoch, *counter;
    KMAN_TRY(kman_lookback_begin(ctx, 1, &epoch, &counter));  // (the chain counter only)
    // count items leave pass 1 as 4 bytes when the narrow finish takes them
    // (KMAN_WIDE_ITEMS=1: 8 bytes, for A/B)
    const bool narrow4 = narrow_ok(ctx, mode, p.Q, p.rest, 0) && !getenv("KMAN_WIDE_ITEMS");
    {
        KTimer kt_(ctx, "region_pass");
        PassArgs pa{};
        pa.in = g.r0;
        pa.seg_base = nullptr;
        pa.seg_cnt = g.c0;
        pa.cnt_sb = 1;  // (rg_extract's cursors: [segment][bucket])
        pa.stride = p.C0;
        pa.nbk = 1u << G1;
        pa.nsg = RS;
        pa.gsub = 1;
        pa.H = p.H;
        pa.shift = p.Q + p.rest;
        pa.bits = p.B2;
        pa.out = g.r1;
        pa.C1 = p.C1h;
        pa.cnt1 = g.c1;
        pa.big = 1;
        pa.lines = 1;
        pa.line1 = getenv("KMAN_PASS_LINE1") ? 1 : 0;
        launch_pass(ctx, pa, counter, stamps[1], false, narrow4);
        HIP_TRY(ctx, hipGetLastError());
    }
    {
        FinishArgs f{g.r1, p.C1h, g.c1, p.Q, p.rest, (uint32_t)p.rc, 0, 0, g.nreg};
        f.fsub = p.H;
        f.in4 = narrow4;
        KMAN_TRY(run_finish(ctx, f, mode, d_okeys, d_ovals, oval_bytes, stamps[2]));
    }
    if (stamps[0]) KMAN_TRY(report_stamps(ctx, stamps, stamp_rows));
    uint64_t *h = ctx->h_small;
    HIP_TRY(ctx, hipMemcpyAsync(h + 4, ctx->d_status + (g.nreg - 1), 8, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(h + 8, ctx->d_err, 4, hipMemcpyDeviceToHost, ctx->stream));
    std::vector<uint32_t> hc((size_t)RS << G1);
    HIP_TRY(ctx, hipMemcpyAsync(hc.data(), g.c0, hc.size() * 4, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    uint32_t e;
    memcpy(&e, h + 8, 4);
    if (e) {
        HIP_TRY(ctx, hipMemsetAsync(ctx->d_err, 0, sizeof(uint32_t), ctx->stream));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        if (e & ERR_REGION) return KMAN_EFALLBACK;  // a region overflowed: outputs invalid, redone elsewhere
        return region_fault(ctx, e, "kman_groups");
    }
    const uint64_t wd = h[4];
    if (((wd >> 56) & 63u) != ctx->epoch || (wd >> 62) != ST_INCL)
        return kman_fail(ctx, KMAN_EHIP, "region output total not published");
    uint64_t nk = 0;
    for (uint32_t v : hc) nk += v;
    *n_kmers = nk;
    *n_out = wd & ST_VMASK;
    return KMAN_OK;
}

}  // namespace

extern "C" int kman_groups(kman_ctx *ctx, const uint8_t *d_codes, uint64_t n_bases, uint32_t k, uint32_t flags,
                           int mode, void *d_work, uint64_t work_bytes, uint64_t *d_okeys, void *d_ovals,
                           uint32_t oval_bytes, uint64_t *n_kmers, uint64_t *n_out) {
    if (!ctx || !n_kmers || !n_out) return KMAN_EINVAL;
    *n_kmers = 0;
    *n_out = 0;
    GroupsCall g;
    KMAN_TRY(groups_setup(ctx, n_bases, k, flags, mode, d_work, work_bytes, &g));
    if (!d_codes) return kman_fail(ctx, KMAN_EINVAL, "null buffer");
    KMAN_TRY(groups_outputs_ok(ctx, g, mode, d_okeys, d_ovals, oval_bytes, n_bases));
    const RegionPlan &p = g.p;
    HIP_TRY(ctx, hipMemsetAsync(g.c0, 0, p.bytes - p.off_c0, ctx->stream));
    uint64_t *stamps[3] = {nullptr, nullptr, nullptr};
    const uint64_t stamp_rows[3] = {p.n_tiles0, (uint64_t)p.maxt1 << G1, g.nreg};
    if (getenv("KMAN_RG_STAMPS"))
        for (int q = 0; q < 3; q++) {
            HIP_TRY(ctx, hipMalloc((void **)&stamps[q], stamp_rows[q] * 128));
            HIP_TRY(ctx, hipMemsetAsync(stamps[q], 0, stamp_rows[q] * 128, ctx->stream));
        }
    uint32_t epoch, *counter;
    // pass 0: extraction by the top 8 bits
    KMAN_TRY(kman_lookback_begin(ctx, 1, &epoch, &counter));  // (the ticket counters only)
    {
        KTimer kt_(ctx, "region_extract");
        launch_extract_any(ctx, p, d_codes, n_bases, k, g.r0, g.c0, epoch, counter, stamps[0]);
        HIP_TRY(ctx, hipGetLastError());
    }
    return groups_tail(ctx, g, mode, d_okeys, d_ovals, oval_bytes, stamps, stamp_rows, n_kmers, n_out);
}

extern "C" int kman_groups_begin(kman_ctx *ctx, uint64_t n_bases, uint32_t k, uint32_t flags, int mode,
                                 void *d_work, uint64_t work_bytes, uint32_t *n_tiles, uint64_t *tile_bases) {
    if (!ctx || !n_tiles || !tile_bases) return KMAN_EINVAL;
    *n_tiles = 0;
    *tile_bases = 0;
    GroupsCall g;
    KMAN_TRY(groups_setup(ctx, n_bases, k, flags, mode, d_work, work_bytes, &g));
    const RegionPlan &p = g.p;
    HIP_TRY(ctx, hipMemsetAsync(g.c0, 0, p.bytes - p.off_c0, ctx->stream));
    uint32_t epoch, *counter;
    KMAN_TRY(kman_lookback_begin(ctx, 1, &epoch, &counter));
    ctx->grp_epoch = epoch;
    ctx->grp_next = 0;
    ctx->grp_tiles = p.n_tiles0;
    *n_tiles = p.n_tiles0;
    *tile_bases = (uint64_t)RT * p.ei;
    return KMAN_OK;
}

namespace {
int groups_extract_to(kman_ctx *ctx, const GroupsCall &g, const uint8_t *d_codes, uint64_t n_bases, uint32_t k,
                      uint32_t tile_hi) {
    const RegionPlan &p = g.p;
    if (ctx->grp_epoch == 0 || ctx->grp_epoch != ctx->epoch || ctx->grp_tiles != p.n_tiles0)
        return kman_fail(ctx, KMAN_EINVAL, "kman_groups_extract: no kman_groups_begin of this input before it, or "
                                           "another look-back call in between");
    if (!d_codes) return kman_fail(ctx, KMAN_EINVAL, "null buffer");
    if (tile_hi > p.n_tiles0) tile_hi = p.n_tiles0;
    uint32_t *counter = ctx->d_counters + ctx->grp_epoch;
    if (tile_hi <= ctx->grp_next) return KMAN_OK;
    {
        KTimer kt_(ctx, "region_extract");
        launch_extract_any(ctx, p, d_codes, n_bases, k, g.r0, g.c0, ctx->grp_epoch, counter, nullptr,
                           tile_hi - ctx->grp_next);
        HIP_TRY(ctx, hipGetLastError());
    }
    ctx->grp_next = tile_hi;
    return KMAN_OK;
}
}  // namespace

extern "C" int kman_groups_extract(kman_ctx *ctx, const uint8_t *d_codes, uint64_t n_bases, uint32_t k,
                                   uint32_t flags, int mode, void *d_work, uint64_t work_bytes, uint32_t tile_hi) {
    if (!ctx) return KMAN_EINVAL;
    GroupsCall g;
    KMAN_TRY(groups_setup(ctx, n_bases, k, flags, mode, d_work, work_bytes, &g));
    return groups_extract_to(ctx, g, d_codes, n_bases, k, tile_hi);
}

extern "C" int kman_groups_end(kman_ctx *ctx, const uint8_t *d_codes, uint64_t n_bases, uint32_t k, uint32_t flags,
                               int mode, void *d_work, uint64_t work_bytes, uint64_t *d_okeys, void *d_ovals,
                               uint32_t oval_bytes, uint64_t *n_kmers, uint64_t *n_out) {
    if (!ctx || !n_kmers || !n_out) return KMAN_EINVAL;
    *n_kmers = 0;
    *n_out = 0;
    GroupsCall g;
    KMAN_TRY(groups_setup(ctx, n_bases, k, flags, mode, d_work, work_bytes, &g));
    KMAN_TRY(groups_outputs_ok(ctx, g, mode, d_okeys, d_ovals, oval_bytes, n_bases));
    KMAN_TRY(groups_extract_to(ctx, g, d_codes, n_bases, k, g.p.n_tiles0));
    ctx->grp_epoch = 0;
    uint64_t *stamps[3] = {nullptr, nullptr, nullptr};
    const uint64_t stamp_rows[3] = {0, 0, 0};
    return groups_tail(ctx, g, mode, d_okeys, d_ovals, oval_bytes, stamps, stamp_rows, n_kmers, n_out);
}

namespace {
// KMAN_RG_VERBOSE: synchronise after each pass of kman_dgroups_finish and
// report which one raised a region overflow (diagnostics only)
int rg_check(kman_ctx *ctx, const char *what, const uint32_t *cnt = nullptr, uint64_t n = 0) {
    static const bool verbose = getenv("KMAN_RG_VERBOSE") != nullptr;
    if (!verbose) return KMAN_OK;
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    uint32_t e = 0;
    HIP_TRY(ctx, hipMemcpy(&e, ctx->d_err, 4, hipMemcpyDeviceToHost));
    uint64_t mx = 0, sum = 0, nz = 0;
    if (cnt && n) {
        std::vector<uint32_t> h(n);
        HIP_TRY(ctx, hipMemcpy(h.data(), cnt, n * 4, hipMemcpyDeviceToHost));
        for (uint32_t v : h) {
            mx = v > mx ? v : mx;
            sum += v;
            nz += v != 0;
        }
        // nonzero counts per block of n/16 entries
        fprintf(stderr, "  nonzero per 1/16:");
        for (int q = 0; q < 16; q++) {
            uint64_t z = 0;
            for (uint64_t i = q * n / 16; i < (q + 1) * n / 16; i++) z += h[i] != 0;
            fprintf(stderr, " %llu", (unsigned long long)z);
        }
        fprintf(stderr, "\n  first 8:");
        for (int q = 0; q < 8 && q < (int)n; q++) fprintf(stderr, " %u", h[q]);
        fprintf(stderr, "\n");
    }
    fprintf(stderr, "kman_dgroups: after %s err=%u counts n=%llu nonzero=%llu sum=%llu max=%llu\n", what, e,
            (unsigned long long)n, (unsigned long long)nz, (unsigned long long)sum, (unsigned long long)mx);
    return KMAN_OK;
}
}  // namespace

// =============================================================== N > 1
// The region path across G ranks, in key rounds (one process per GPU;
// kman_amd/dist.py drives the collectives between the calls).  Each rank holds
// one byte-range shard of the FASTA (codes + a (k-1)-base halo):
//   kman_dshard_hist     exact item counts per (top-8-bit bucket b, position
//                        segment s) of the shard, in rg_extract's tile geometry
//   (host)               all-gather of the per-bucket counts; the 256 buckets
//                        cut into G x R contiguous parts of ~equal k-mers:
//                        rank q owns parts q*R .. q*R+R-1, round r handles part
//                        q*R + r of every rank q, so a rank's rounds produce
//                        its key range in order and the ranks' outputs in
//                        rank order are the global output
//   per round r:
//   kman_dshard_extract  pass 0 of the shard over the round's buckets only,
//                        written straight into the send buffer: region (b, s)
//                        at rtab[b * RS + s] (exact, destination-major, so no
//                        gather pass and no padding)
//   (host)               one all-to-all of the packed items (RCCL, xGMI)
//   kman_dround_finish   per (bucket, source) chain: pass 1 by 9 bits into
//                        sub-regions (b, d, src, h); pass 1b per (b, d) by g
//                        more bits (g >= ceil(log2 G), more when the round's
//                        buckets are large), tagging each item with its source
//                        rank in the now implied d field; then the LDS finish,
//                        appending the round's rows to the rank's output.
// Uniq pos carry the source rank in bits 56-63.  The round working set is
// two arenas: A = the send buffer, then pass-1 sub-regions; B = the receive
// buffer, then pass-1b regions (the receive buffer is dead after pass 1).
namespace {

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

// the shard's pass-0 geometry (rg_extract / rg_hist): no capacity limits,
// no region area (the exact layout needs none); Q from the common bound
int make_shard_plan(uint64_t n_bases, uint64_t n_bases_q, uint32_t k, uint32_t flags, int mode, RegionPlan *pl) {
    if (mode != KMAN_FINISH_COUNT && mode != KMAN_FINISH_UNIQ) return KMAN_EINVAL;
    if (k < 2 || k > 32 || n_bases_q < n_bases) return KMAN_EINVAL;
    if (getenv("KMAN_NO_REGION")) return KMAN_EFALLBACK;
    if (mode == KMAN_FINISH_UNIQ && k > 25) return KMAN_EFALLBACK;  // (the tile-local window index above the key)
    RegionPlan p{};
    p.canon = flags & KMAN_CANONICAL;
    p.mix = p.canon && (flags & KMAN_MIXED);
    p.rc = (flags & KMAN_RC) && !p.canon;
    p.K = 2 * k;
    if (p.K < B1 + 9 + 1) return KMAN_EFALLBACK;  // (the rounds' passes need 8 + 9 key bits and one more)
    p.W = n_bases * (p.rc ? 2 : 1);
    const uint64_t Wq = n_bases_q * (p.rc ? 2 : 1);
    p.Q = mode == KMAN_FINISH_UNIQ ? (bitlen(Wq - 1) ? bitlen(Wq - 1) : 1u) : 0u;
    if (p.K - B1 + p.Q > 64) return KMAN_EFALLBACK;
    // the shard extraction's tiles (rg_hist counts in the same geometry): 16
    // windows per thread (8 with -r) for shards that one key round takes
    // (1 GB per rank: 2.80-2.88 vs 3.05-3.45 ms with 12), 12 (6) for the big
    // ones, whose rounds keep 1/R of the windows each (config 4's 12.5 GB:
    // 63.8-64.2 vs 71.8-72.2 ms with 16, `r04aj_tiles_ab.txt`); decided on
    // the common bound, so every rank takes the same
    // (KMAN_ONCE: every window of the shard is kept by one extraction for all
    // rounds, so the 16-window tiles as well)
    const bool wide = n_bases_q <= (4ull << 30) || (flags & KMAN_ONCE);
    p.ei = p.rc ? (wide ? 8u : 6u) : (wide ? 16u : 12u);
    const uint64_t win = (uint64_t)RT * p.ei;
    p.n_tiles0 = (uint32_t)ceil_div(n_bases ? n_bases : 1, win);
    p.seg_tiles = (uint32_t)ceil_div(p.n_tiles0, RS);
    *pl = p;
    return KMAN_OK;
}

struct RoundPlan {
    uint32_t K, Q, g, rest, G, nb;
    uint32_t H;           // pass-1 chains per (bucket, source)
    bool p1b;             // pass 1b runs (by g >= 0 bits); else the finish reads pass 1's sub-regions
    bool rc;
    uint64_t C1s, C1;     // pass-1 sub-region / pass-1b region capacities
    int cap;              // the finish's capacity: GCAP when the planned regions fit it (three blocks per CU)
    uint64_t nsub, nreg;
    // arena A: r1 | c1 | pass-1 segment bases (u64) + counts (u32) | region
    // overflow flags (u8); arena B: r2 | c2
    uint64_t off_c1, off_tab, off_fail, a_bytes, off_c2, b_bytes;
};

// Capacity of a region that expects e items: e + max(e / 8, 8 sd of a
// Poisson fill) -- the round path's arenas are most of a rank's HBM, and at
// config 4's size (12.5 G k-mers per rank) a 1.5 x slack cost one key round (a
// re-read and re-roll of the whole shard).  A region that overflows anyway (a
// repeat) is redone by key range.
uint64_t round_cap(uint64_t e, uint64_t extra) {
    const uint64_t sd8 = (uint64_t)(8.0 * sqrt((double)e)) + 1;
    return ceil_div(e + (e / 8 > sd8 ? e / 8 : sd8) + extra, 64) * 64;
}

// counts[src * nb + j] = items of bucket b_lo + j from rank src
int make_rplan(uint32_t k, uint32_t flags, int mode, uint32_t world, uint64_t n_bases_q, uint32_t nb,
               const uint64_t *counts, RoundPlan *rp) {
    if (mode != KMAN_FINISH_COUNT && mode != KMAN_FINISH_UNIQ) return KMAN_EINVAL;
    if (k < 2 || k > 32 || world < 1 || world > 32 || nb > (uint32_t)RADIX) return KMAN_EINVAL;
    if (nb && !counts) return KMAN_EINVAL;
    RoundPlan d{};
    const bool canon = flags & KMAN_CANONICAL;
    d.rc = (flags & KMAN_RC) && !canon;
    d.K = 2 * k;
    d.G = world;
    d.nb = nb;
    const uint64_t Wq = n_bases_q * (d.rc ? 2 : 1);
    d.Q = mode == KMAN_FINISH_UNIQ ? (bitlen(Wq - 1) ? bitlen(Wq - 1) : 1u) : 0u;
    if (d.K - B1 + d.Q > 64) return KMAN_EFALLBACK;
    uint64_t maxsb = 0, maxb = 0;  // largest (bucket, source) chunk, largest bucket
    for (uint32_t j = 0; j < nb; j++) {
        uint64_t t = 0;
        for (uint32_t src = 0; src < world; src++) {
            const uint64_t c = counts[(uint64_t)src * nb + j];
            if (c > 0xffffffffull) return KMAN_EFALLBACK;  // (pass-1 chain lengths are u32)
            maxsb = c > maxsb ? c : maxsb;
            t += c;
        }
        maxb = t > maxb ? t : maxb;
    }
    // pass 1: H block-owned chains per (bucket, source), enough chains to
    // fill the CUs (a round of few buckets on few ranks has few chains);
    // pass 1b concatenates the G * H sub-regions of a (b, d): at most 64
    // H: the fewest chains with the shortest makespan on the 256 CUs (one
    // 1024-thread pass block each): ceil(nb G H / 256) / H bucket-chunks per
    // CU -- 85 buckets take H = 3 (255 chains), not 4 (340: a second wave of
    // 84 chains on 84 CUs, pass 1 19.7 vs 10.1 ms per config-4 round)
    {
        const uint64_t ch1 = (uint64_t)nb * world;
        d.H = 2;
        double best = 1e30;
        for (uint32_t h = 2; h <= 16 && world * h <= 64; h++) {
            const double ms = (double)ceil_div(ch1 * h, 256) / h;
            if (ms < best * 0.95) {  // (more chains only for a clear gain)
                best = ms;
                d.H = h;
            }
        }
    }
    // pass 1b bits g: until a final region expects <= FFILL_T items (the
    // LDS finish holds FCAP = 8704).  g = 0 (no pass 1b, the finish reads the
    // pass-1 sub-regions) when one rank's 9-bit regions already fit: with one
    // source and two chains (N > 1 needs pass 1b anyway, to tag each item with
    // its source rank for uniq and to merge the ranks' sub-regions)
    // Pass 1b runs whenever the finish cannot read the pass-1 sub-regions
    // itself (more than two per region: N > 1, or H > 2) -- with g = 0 bits
    // (a pass that only merges the sources' sub-regions and tags uniq items
    // with their rank) while a (b, d) region's expected fill is <= FFILL_M,
    // as kman_groups keeps its 17-bit regions: N > 1 at 1 G k-mers per rank
    // then finishes ~7.6 K-item regions, not twice as many of half the size
    // (finish 6.3 vs 5.3 ms per 1 G uniq k-mers at world 1, KMAN_DROUND_P1B)
    uint32_t g = 0;
    {
        const char *e = getenv("KMAN_DROUND_MIN_G");  // tests: the wide pass-1b digits of huge rounds
        g = e ? (uint32_t)atoi(e) : 0u;
        g = g <= 9 ? g : 9;
    }
    const uint64_t e2f = maxb >> 9;
    const bool p1b = g > 0 || getenv("KMAN_DROUND_P1B") != nullptr || world * d.H > 2 || e2f > FFILL_M;
    while (p1b && g < 9 && (e2f >> g) > FFILL_T && (g > 0 || e2f > FFILL_M)) g++;
    if ((e2f >> g) > FFILL_M) return KMAN_EFALLBACK;
    d.p1b = p1b;
    if (d.K < B1 + 9 + g + 1) return KMAN_EFALLBACK;
    d.g = g;
    d.rest = d.K - B1 - 9 - g;
    const uint64_t e1 = maxsb / (512ull * d.H);
    d.C1s = round_cap((flags & KMAN_ROOMY) ? 2 * e1 : e1, 256);
    if ((uint64_t)512 * world * d.H * d.C1s >= (1ull << 31)) return KMAN_EFALLBACK;  // (32-bit WC offsets)
    const uint64_t e2 = (maxb >> 9) >> g;
    const uint64_t c2 = round_cap(e2, 512);
    d.C1 = c2 < (uint64_t)FCAP ? c2 : (uint64_t)FCAP;
    // the finish at GCAP (40 KiB, three blocks per CU) when the regions the
    // plan expects fit it with the same margin; else FCAP (68 KiB, two)
    d.cap = round_cap(e2, 512) <= (uint64_t)GCAP ? GCAP : FCAP;
    if (d.cap == GCAP) d.C1 = d.C1 < (uint64_t)GCAP ? d.C1 : (uint64_t)GCAP;
    d.nsub = (uint64_t)nb * 512 * world * d.H;
    d.nreg = (uint64_t)nb * 512 << g;
    d.off_c1 = d.nsub * d.C1s * 8;
    d.off_tab = ceil_div(d.off_c1 + d.nsub * 4, 64) * 64;
    d.off_fail = d.off_tab + ceil_div((uint64_t)nb * world * 12 + 64, 64) * 64;
    d.a_bytes = d.off_fail + ceil_div(d.nreg + 64, 64) * 64;
    d.off_c2 = p1b ? d.nreg * d.C1 * 8 : 0;
    d.b_bytes = p1b ? d.off_c2 + ceil_div(d.nreg * 4 + 64, 64) * 64 : 64;
    *rp = d;
    return KMAN_OK;
}

int read_err(kman_ctx *ctx, uint32_t *e) {
    HIP_TRY(ctx, hipMemcpyAsync(ctx->h_small + 8, ctx->d_err, 4, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    memcpy(e, ctx->h_small + 8, 4);
    if (*e) {
        HIP_TRY(ctx, hipMemsetAsync(ctx->d_err, 0, 4, ctx->stream));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        if (*e != ERR_REGION) return region_fault(ctx, *e, "kman_dround_finish");
    }
    return KMAN_OK;
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

// Pass 1b's width g, refitted from the pass-1 counts.  The plan takes g from
// the largest bucket, and a genome's repeats inflate every bucket that holds
// one (a satellite k-mer with 10^5 copies): g = 4 instead of 2 on the
// GRCh38-shaped input, 2 M finish regions of 1.4 K items where per-region
// costs dominate (16.6 us per region at 1.4 K items, 20 us at 3.8 K).  Here g
// covers all but the largest 0.5 % of the (b, d) sub-buckets (the ones a
// repeat fills, which overflow at any g and are redone by key range), never
// above the plan's.  Pass 1 flagged overflowing sub-buckets per (b, d);
// they are spread over their 2^g regions here.
int refit_g(kman_ctx *ctx, RoundPlan &d, const uint32_t *c1, uint8_t *freg, uint32_t G, bool *p1_lost) {
    const uint64_t nbd = (uint64_t)d.nb * 512, gh = (uint64_t)G * d.H;
    std::vector<uint32_t> hc(d.nsub);
    std::vector<uint8_t> hf(nbd);
    HIP_TRY(ctx, hipMemcpyAsync(hc.data(), c1, d.nsub * 4, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(hf.data(), freg, nbd, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    uint32_t gmin = 1;
    if (const char *e = getenv("KMAN_DROUND_MIN_G")) gmin = std::max<uint32_t>(gmin, std::min(9, atoi(e)));
    std::vector<uint8_t> need(nbd);
    std::vector<uint64_t> size(nbd);
    for (uint64_t j = 0; j < nbd; j++) {
        uint64_t t = 0;
        for (uint64_t q = 0; q < gh; q++) t += hc[j * gh + q];
        size[j] = t;
        uint32_t g = gmin;
        while (g < 9 && (t >> g) > FFILL_T) g++;
        need[j] = (uint8_t)g;
    }
    std::vector<uint64_t> ss(size);
    const uint64_t qi = (uint64_t)(0.995 * (double)(nbd - 1));
    std::nth_element(ss.begin(), ss.begin() + qi, ss.end());
    std::vector<uint8_t> ns(need);
    std::nth_element(ns.begin(), ns.begin() + qi, ns.end());
    uint32_t g = std::max<uint32_t>(gmin, ns[qi]);
    if (g < d.g) {
        const uint64_t nreg = nbd << g;
        const uint64_t e2 = ss[qi] >> g;
        uint64_t C1 = std::min<uint64_t>(round_cap(e2, 512), (uint64_t)FCAP);
        C1 = std::max<uint64_t>(C1, d.C1);  // (never tighter than planned)
        C1 = std::min<uint64_t>(C1, (uint64_t)FCAP);
        const uint64_t off_c2 = nreg * C1 * 8;
        if (off_c2 + ceil_div(nreg * 4 + 64, 64) * 64 <= d.b_bytes) {
            d.g = g;
            d.rest = d.K - B1 - 9 - g;
            d.nreg = nreg;
            d.C1 = C1;
            d.cap = C1 <= (uint64_t)GCAP ? GCAP : FCAP;
            d.off_c2 = off_c2;
        }
    }
    // pass 1's (b, d) flags -> the regions they feed
    bool any = false;
    for (uint64_t j = 0; j < nbd; j++) any |= hf[j] != 0;
    *p1_lost = any;
    if (any && getenv("KMAN_DROUND_LOG")) {
        uint64_t nl = 0, big = 0;
        for (uint64_t j = 0; j < nbd; j++)
            if (hf[j]) {
                nl++;
                big = std::max(big, size[j]);
            }
        fprintf(stderr, "refit_g: pass 1 lost items in %llu of %llu sub-buckets (C1s %llu; the largest kept %llu)\n",
                (unsigned long long)nl, (unsigned long long)nbd, (unsigned long long)d.C1s, (unsigned long long)big);
    }
    if (any) {
        std::vector<uint8_t> fr(d.nreg, 0);
        for (uint64_t j = 0; j < nbd; j++)
            if (hf[j]) memset(&fr[j << d.g], 1, (size_t)1 << d.g);
        HIP_TRY(ctx, hipMemcpyAsync(freg, fr.data(), d.nreg, hipMemcpyHostToDevice, ctx->stream));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));  // (fr leaves scope)
    } else {
        HIP_TRY(ctx, hipMemsetAsync(freg, 0, nbd, ctx->stream));
    }
    return KMAN_OK;
}

// ---------------------------------------------------------------- 0-bit pass 1b
// Pass 1b with g = 0 bits is a merge: region r = (b, d) takes the G x H
// pass-1 sub-regions (b, d, src, h) one after another (uniq: each item's d
// field replaced by its source rank, src = segment / H, as rg_pass tags it).
// One block per region, every item placed by its position (the segment from
// a binary search over the <= 64 segment starts in LDS), so a block's loads
// are independent; c2[r] = the region's size, clipped to C1 (past it the
// region is flagged, as rg_pass flags it).
template <typename T>
__global__ __launch_bounds__(256) void rg_merge_regions(const T *__restrict__ in, uint64_t C1s,
                                                        const uint32_t *__restrict__ c1, uint32_t nsg, uint32_t H,
                                                        T *__restrict__ out, uint64_t C1, uint32_t *__restrict__ c2,
                                                        uint8_t *__restrict__ freg, uint32_t *__restrict__ err,
                                                        uint32_t tag, uint32_t tag_shift) {
    __shared__ uint32_t pre[65];
    const uint64_t r = blockIdx.x;
    if (threadIdx.x < 64) {
        const uint32_t c = threadIdx.x < nsg ? c1[r * nsg + threadIdx.x] : 0u;
        const uint32_t inc = wave_inclusive_scan(c, SumU32());
        pre[threadIdx.x] = inc - c;
        if (threadIdx.x == 63) pre[64] = inc;
    }
    __syncthreads();
    const uint32_t tot = pre[64];
    const uint32_t lim = tot < C1 ? tot : (uint32_t)C1;
    if (threadIdx.x == 0) {
        c2[r] = lim;
        if (tot > C1) {
            freg[r] = 1;
            atomicOr(err, ERR_REGION);
        }
    }
    const uint64_t tm = tag ? 0x1ffull << tag_shift : 0ull;
    T *const dst = out + r * C1;
#pragma unroll 4
    for (uint32_t p = threadIdx.x; p < lim; p += 256) {
        uint32_t lo = 0, hi = nsg;  // the last segment starting at or before p
        while (hi - lo > 1) {
            const uint32_t mid = (lo + hi) >> 1;
            if (pre[mid] <= p) lo = mid;
            else hi = mid;
        }
        T v = in[(r * nsg + lo) * C1s + (p - pre[lo])];
        if (tag) v = (T)(((uint64_t)v & ~tm) | ((uint64_t)(lo / H) << tag_shift));
        dst[p] = v;
    }
}

// ---------------------------------------------------------------- heavy keys
// A key round's heavy keys (PassArgs::hv_tab): every S-th received item's
// full key is sampled, the samples sorted and run-length counted, and the
// keys sampled at least twice (so they occur at least twice: a uniq round may
// drop all their copies) -- the most often sampled, at most HV_BMAX per bucket --
// go into an open-addressing table that pass 1 probes per item.  Pass 1 adds
// each key's dropped copies to drop[slot]; rg_hv_fix then adds them to the
// key's row (count mode: pass 1 kept one copy per chain, so the row exists
// unless its region was left out, in which case the partial redo recounts
// the whole key range from the codes).

// sample i = the item at i * S; runs (src, j) lie in src-major order, run t =
// src * nb + j starting at rs[t] (the last run starting at or before p holds p)
__global__ __launch_bounds__(256) void rg_hv_sample(const uint64_t *__restrict__ in, const uint64_t *__restrict__ rs,
                                                    uint32_t nrun, uint32_t nb, uint64_t S, uint64_t ns, uint32_t b_lo,
                                                    uint32_t kb, uint32_t q, uint64_t *__restrict__ out) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= ns) return;
    const uint64_t p = i * S;
    uint32_t lo = 0, hi = nrun;
    while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) >> 1;
        if (rs[mid] <= p) lo = mid;
        else hi = mid;
    }
    out[i] = ((uint64_t)(b_lo + lo % nb) << kb) | (in[p] >> q);
}

// One block per bucket j of the round: its sampled keys (the run-length
// output ukeys / cnt, sorted) seen >= 2 times, the most often sampled of them
// (hits >= a cut-off that leaves <= HV_BMAX; the first HV_BMAX in key order
// when more than that were sampled >= 63 times) into the bucket's table of key
// rests (an LDS open-addressing table of HV_BSLOTS, filled by CAS, then
// written out with each slot's index j * HV_BMAX + i into keys), *total +=
// the keys taken
__global__ __launch_bounds__(256) void rg_hv_build(const uint64_t *__restrict__ ukeys, const uint32_t *__restrict__ cnt,
                                                   uint64_t nu, uint32_t b_lo, uint32_t kb, uint64_t *__restrict__ tab,
                                                   uint32_t *__restrict__ idx, uint64_t *__restrict__ keys,
                                                   uint32_t *__restrict__ total) {
    __shared__ unsigned long long t_[HV_BSLOTS];
    __shared__ uint32_t ti[HV_BSLOTS];
    __shared__ uint32_t hist[64], wsum[4], s_cut;
    __shared__ uint64_t s_lo, s_hi;
    const uint32_t j = blockIdx.x, tid = threadIdx.x;
    const int lane = lane_id(), w = tid >> 6;
    for (uint32_t q = tid; q < HV_BSLOTS; q += 256) {
        t_[q] = HV_EMPTY;
        ti[q] = 0;
    }
    if (tid < 64) hist[tid] = 0;
    if (tid < 2) {  // the bucket's range [lo, hi) of ukeys
        const uint64_t want = (uint64_t)(b_lo + j + tid) << kb;
        uint64_t lo = 0, hi = nu;
        while (lo < hi) {
            const uint64_t mid = (lo + hi) >> 1;
            if (ukeys[mid] < want) lo = mid + 1;
            else hi = mid;
        }
        if (tid == 0) s_lo = lo;
        else s_hi = lo;
    }
    __syncthreads();
    const uint64_t lo = s_lo, hi = s_hi;
    for (uint64_t i = lo + tid; i < hi; i += 256) {
        const uint32_t c = cnt[i];
        if (c >= 2) atomicAdd(&hist[c < 63 ? c : 63], 1u);
    }
    __syncthreads();
    if (tid == 0) {
        uint32_t above = 0, cut = 64;
        for (uint32_t t = 63; t >= 2; t--) {
            if (above + hist[t] > HV_BMAX) break;
            above += hist[t];
            cut = t;
        }
        s_cut = cut == 64 && hist[63] ? 63 : cut;  // (64: none)
    }
    __syncthreads();
    const uint32_t cut = s_cut;
    // the keys >= cut in key order, 256 at a time (cut 64: none; the
    // bucket's table and keys are written empty all the same -- they hold a
    // previous round's otherwise)
    uint32_t base = 0;
    for (uint64_t c0 = lo; cut < 64 && c0 < hi && base < HV_BMAX; c0 += 256) {
        const uint64_t i = c0 + tid;
        const bool take = i < hi && cnt[i] >= cut;
        const uint64_t m = __ballot(take);
        if (lane == 0) wsum[w] = (uint32_t)__popcll(m);
        __syncthreads();
        uint32_t before = 0, tot = 0;
        for (int q = 0; q < 4; q++) {
            before += q < w ? wsum[q] : 0u;
            tot += wsum[q];
        }
        const uint32_t at = base + before + (uint32_t)__popcll(m & lanemask_lt());
        if (take && at < HV_BMAX) {
            const uint64_t key = ukeys[i], kr = key & ((1ull << kb) - 1);
            uint32_t sl = hv_slot(kr);
            while (atomicCAS(&t_[sl], (unsigned long long)HV_EMPTY, (unsigned long long)kr) != HV_EMPTY)
                sl = (sl + 1) & (HV_BSLOTS - 1);
            ti[sl] = j * HV_BMAX + at;
            keys[(uint64_t)j * HV_BMAX + at] = key;
        }
        base += tot;
        __syncthreads();
    }
    const uint32_t n = base < HV_BMAX ? base : HV_BMAX;
    for (uint32_t q = n + tid; q < HV_BMAX; q += 256) keys[(uint64_t)j * HV_BMAX + q] = HV_EMPTY;
    for (uint32_t q = tid; q < HV_BSLOTS; q += 256) {
        tab[(uint64_t)j * HV_BSLOTS + q] = t_[q];
        idx[(uint64_t)j * HV_BSLOTS + q] = ti[q];
    }
    if (tid == 0) atomicAdd(total, n);
}

// each heavy key's dropped copies onto its row (rows sorted by key)
template <typename V>
__global__ __launch_bounds__(256) void rg_hv_fix(const uint64_t *__restrict__ keys, const uint64_t *__restrict__ drop,
                                                 uint32_t m, const uint64_t *__restrict__ okeys, V *__restrict__ ovals,
                                                 uint64_t n) {
    const uint32_t s = blockIdx.x * 256 + threadIdx.x;
    if (s >= m) return;
    const uint64_t key = keys[s], d = drop[s];
    if (!d || !n || key == HV_EMPTY) return;
    uint64_t lo = 0, hi = n;  // first row >= key
    while (lo < hi) {
        const uint64_t mid = (lo + hi) >> 1;
        if (okeys[mid] < key) lo = mid + 1;
        else hi = mid;
    }
    if (lo < n && okeys[lo] == key) ovals[lo] += (V)d;
}

// kman_dround_left: the items of the left-out regions, from the pass-1
// sub-regions (bd, src, h) = subs[i] of their sub-buckets bd (a sub-bucket's
// 2^g regions are left out one by one: an item is kept when freg flags its
// region) as full keys (+ uniq pos, as the finish emits them).  Block
// (i, y) takes the sub-region's 2048-item chunks y, y + Y, ...; WRITE = false
// counts its items into bcnt[block], WRITE = true writes them from
// boff[block] on (a scan of those counts), in chunk order
template <typename TI, bool WRITE>
__global__ __launch_bounds__(256) void rg_left_gather(const TI *__restrict__ r1, uint64_t C1s,
                                                      const uint32_t *__restrict__ subs,
                                                      const uint32_t *__restrict__ cnts, const uint8_t *__restrict__ freg,
                                                      uint32_t g, uint32_t G, uint32_t H, uint32_t b_lo, uint32_t kb,
                                                      uint32_t Q, uint32_t rc, uint64_t *__restrict__ bco,
                                                      uint64_t *__restrict__ okeys, uint64_t *__restrict__ opos) {
    constexpr int E = 8;
    __shared__ uint32_t wsum[4];
    const uint32_t i = blockIdx.x, bid = blockIdx.x * gridDim.y + blockIdx.y;
    const uint32_t s = subs[i], n = cnts[i];
    const uint32_t bd = s / (G * H), src = (s / H) % G;
    const uint64_t hi = (uint64_t)(b_lo + (bd >> 9)) << kb;
    const uint64_t kmask = (1ull << kb) - 1, qmask = Q ? (1ull << Q) - 1 : 0ull;
    const uint32_t rsh = kb - 9 - g;  // key bits below the region
    const TI *in = r1 + (uint64_t)s * C1s;
    const int lane = lane_id(), w = threadIdx.x >> 6;
    uint64_t base = WRITE ? bco[bid] : 0;
    uint32_t mine = 0;
    for (uint32_t c0 = blockIdx.y * 256 * E; c0 < n; c0 += gridDim.y * 256 * E) {
        uint64_t kk[E], vv[E];
        uint32_t km = 0;
#pragma unroll
        for (int e = 0; e < E; e++) {
            const uint32_t j = c0 + e * 256 + threadIdx.x;
            kk[e] = vv[e] = 0;
            if (j < n) {
                const uint64_t v = in[j];
                uint64_t key;
                if constexpr (sizeof(TI) == 4) key = hi | ((uint64_t)(bd & 511u) << (kb - 9)) | (v & ((1ull << (kb - 9)) - 1));
                else key = hi | ((v >> Q) & kmask);
                const uint64_t r = ((uint64_t)bd << g) | ((key >> rsh) & ((1ull << g) - 1));
                if (freg[r]) km |= 1u << e;
                kk[e] = key;
                vv[e] = v;
            }
        }
        const uint32_t c = (uint32_t)__popc(km);
        if constexpr (!WRITE) {
            mine += c;
            continue;
        }
        // the chunk's block-wide exclusive offsets
        const uint32_t inc = wave_inclusive_scan(c, SumU32());
        if (lane == 63) wsum[w] = inc;
        __syncthreads();
        uint32_t before = 0, tot = 0;
#pragma unroll
        for (int q = 0; q < 4; q++) {
            before += q < w ? wsum[q] : 0u;
            tot += wsum[q];
        }
        __syncthreads();
        uint64_t at = base + before + inc - c;
#pragma unroll
        for (int e = 0; e < E; e++) {
            if (!((km >> e) & 1u)) continue;
            okeys[at] = kk[e];
            if (sizeof(TI) == 8 && opos) {
                const uint64_t idx = vv[e] & qmask;
                opos[at] = (rc ? idx : idx << 1) | ((uint64_t)src << 56);
            }
            at++;
        }
        base += tot;
    }
    if constexpr (!WRITE) {
        const uint32_t inc = wave_inclusive_scan(mine, SumU32());
        if (lane == 63) wsum[w] = inc;
        __syncthreads();
        if (threadIdx.x == 0) bco[bid] = (uint64_t)wsum[0] + wsum[1] + wsum[2] + wsum[3];
    }
}

__global__ __launch_bounds__(256) void rg_left_counts(const uint32_t *__restrict__ c1, const uint32_t *__restrict__ subs,
                                                      uint32_t n, uint64_t C1s, uint32_t *__restrict__ cnts) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) {
        const uint32_t c = c1[subs[i]];
        cnts[i] = c < C1s ? c : (uint32_t)C1s;
    }
}

struct HeavyRound {
    uint32_t n = 0;  // heavy keys in the table (0: none, pass 1 as usual)
    uint32_t slots = 0;  // the keys list's length (HV_BMAX per bucket, HV_EMPTY where unused)
    char *w = nullptr;  // kman_ctx::d_hv (HVO_* parts)
};

int hv_fix(kman_ctx *ctx, const char *w, uint32_t m, const uint64_t *okeys, void *ovals, uint32_t vb, uint64_t n) {
    const uint64_t *keys = (const uint64_t *)(w + HVO_KEYS), *drop = (const uint64_t *)(w + HVO_DROP);
    const dim3 grid((m + 255) / 256);
    if (vb == 4)
        hipLaunchKernelGGL(rg_hv_fix<uint32_t>, grid, dim3(256), 0, ctx->stream, keys, drop, m, okeys,
                           (uint32_t *)ovals, n);
    else
        hipLaunchKernelGGL(rg_hv_fix<uint64_t>, grid, dim3(256), 0, ctx->stream, keys, drop, m, okeys,
                           (uint64_t *)ovals, n);
    HIP_TRY(ctx, hipGetLastError());
    return KMAN_OK;
}

int hv_buffer(kman_ctx *ctx, size_t bytes, char **p) {
    if (bytes > ctx->hv_bytes) {
        if (ctx->d_hv) {
            HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
            HIP_TRY(ctx, hipFree(ctx->d_hv));
            ctx->d_hv = nullptr;
            ctx->hv_bytes = 0;
        }
        HIP_TRY(ctx, hipMalloc(&ctx->d_hv, bytes));
        ctx->hv_bytes = bytes;
    }
    *p = (char *)ctx->d_hv;
    return KMAN_OK;
}

// The round's heavy keys (see above).  hb[j * G + src] = run (j, src)'s start
// in d_recv, total = the round's items.  KMAN_HEAVY=0 turns it off.
int find_heavy(kman_ctx *ctx, const RoundPlan &d, const uint64_t *d_recv, const std::vector<uint64_t> &hb,
               uint64_t total, uint32_t b_lo, HeavyRound *hv) {
    hv->n = 0;
    const char *e = getenv("KMAN_HEAVY");  // "0": off; "1": any round (tests); else rounds of >= 2^20 items
    if (e && !strcmp(e, "0")) return KMAN_OK;
    const bool force = e && !strcmp(e, "1");
    if (d.K > 62 || (!force && total < (1u << 20)) || !total) return KMAN_OK;  // (table keys < HV_EMPTY)
    const uint32_t nb = d.nb, G = d.G, nrun = nb * G;
    // samples: every S-th item, S >= 64, at most HV_NS
    const uint64_t HV_NS = 1ull << 23;
    const uint64_t S = std::max<uint64_t>(64, ceil_div(total, HV_NS));
    const uint64_t ns = ceil_div(total, S);
    const size_t o_misc = HVO_END, o_rs = o_misc + 512, o_s = o_rs + ceil_div(nrun * 8, 256) * 256, o_a = o_s + ns * 8, o_u = o_a + ns * 8, o_c = o_u + ns * 8,
                 bytes = o_c + ns * 4 + 256;
    char *w;
    KMAN_TRY(hv_buffer(ctx, bytes, &w));
    uint64_t *rs = (uint64_t *)(w + o_rs), *smp = (uint64_t *)(w + o_s), *alt = (uint64_t *)(w + o_a),
             *uk = (uint64_t *)(w + o_u);
    uint32_t *uc = (uint32_t *)(w + o_c);
    std::vector<uint64_t> hrs(nrun);
    for (uint32_t src = 0; src < G; src++)
        for (uint32_t j = 0; j < nb; j++) hrs[(size_t)src * nb + j] = hb[(size_t)j * G + src];
    HIP_TRY(ctx, hipMemcpyAsync(rs, hrs.data(), nrun * 8, hipMemcpyHostToDevice, ctx->stream));
    // the samples sorted and run-length counted: first 2^16 of them (every
    // S1-th item; all distinct -- uniform keys -- ends it here), then ns
    uint64_t nu = 0;
    const auto t0 = std::chrono::steady_clock::now();
    auto ms_since = [&](std::chrono::steady_clock::time_point a) {
        return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - a).count();
    };
    for (int stage = 0; stage < 2; stage++) {
        const uint64_t S_ = stage ? S : std::max<uint64_t>(S, ceil_div(total, 1ull << 16)),
                       ns_ = stage ? ns : ceil_div(total, S_);
        if (stage && S_ == std::max<uint64_t>(S, ceil_div(total, 1ull << 16))) break;  // (stage 0 took them all)
        {
            KTimer kt_(ctx, "heavy_sample");
            hipLaunchKernelGGL(rg_hv_sample, dim3((uint32_t)ceil_div(ns_, 256)), dim3(256), 0, ctx->stream, d_recv,
                               rs, nrun, nb, S_, ns_, b_lo, d.K - B1, d.Q, smp);
            HIP_TRY(ctx, hipGetLastError());
        }
        int in_alt = 0;
        KMAN_TRY(kman_sort(ctx, smp, alt, nullptr, nullptr, 0, ns_, d.K, nullptr, &in_alt));
        KMAN_TRY(kman_rle_count(ctx, in_alt ? alt : smp, ns_, uk, uc, 4, &nu));  // (synchronises)
        if (nu == ns_) return KMAN_OK;  // every sample distinct: no heavy key
    }
    const double t_sort = ms_since(t0);
    const auto t1 = std::chrono::steady_clock::now();
    // the tables built on the device (the buckets without a key sampled
    // twice get empty ones: their chains probe and find nothing)
    uint32_t *d_total = (uint32_t *)(w + o_misc);
    HIP_TRY(ctx, hipMemsetAsync(d_total, 0, 4, ctx->stream));
    HIP_TRY(ctx, hipMemsetAsync(w + HVO_DROP, 0, HV_MAX * 8, ctx->stream));
    hipLaunchKernelGGL(rg_hv_build, dim3(nb), dim3(256), 0, ctx->stream, uk, uc, nu, b_lo, d.K - B1,
                       (uint64_t *)(w + HVO_TAB), (uint32_t *)(w + HVO_IDX), (uint64_t *)(w + HVO_KEYS), d_total);
    HIP_TRY(ctx, hipGetLastError());
    uint32_t m = 0;
    HIP_TRY(ctx, hipMemcpyAsync(&m, d_total, 4, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    if (getenv("KMAN_DROUND_LOG"))
        fprintf(stderr, "find_heavy: %llu samples, %llu distinct, %u keys; sample + sort %.2f ms, tables %.2f\n",
                (unsigned long long)ns, (unsigned long long)nu, m, t_sort, ms_since(t1));
    if (!m) return KMAN_OK;
    hv->n = m;
    hv->slots = nb * HV_BMAX;
    hv->w = w;
    return KMAN_OK;
}

}  // namespace

extern "C" int kman_dshard_plan(uint64_t n_bases, uint64_t n_bases_q, uint32_t k, uint32_t flags, int mode) {
    RegionPlan p;
    return make_shard_plan(n_bases, n_bases_q, k, flags, mode, &p);
}

extern "C" int kman_dshard_hist(kman_ctx *ctx, const uint8_t *d_codes, uint64_t n_bases, uint64_t n_bases_q,
                                uint32_t k, uint32_t flags, int mode, uint32_t *d_hist, uint32_t *hist) {
    if (!ctx || !d_hist || !hist) return KMAN_EINVAL;
    RegionPlan p;
    const int pr = make_shard_plan(n_bases, n_bases_q, k, flags, mode, &p);
    if (pr == KMAN_EINVAL) return kman_fail(ctx, KMAN_EINVAL, "kman_dshard_hist: bad arguments");
    if (pr != KMAN_OK) return pr;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipMemsetAsync(d_hist, 0, (size_t)RADIX * RS * 4, ctx->stream));
    if (n_bases) {
        if (!d_codes) return kman_fail(ctx, KMAN_EINVAL, "null codes");
        KTimer kt_(ctx, "shard_hist");
        if (p.ei == 16 || p.ei == 8) {
            if (p.canon && p.mix) launch_hist<16, false, 2>(ctx, p, d_codes, n_bases, k, d_hist);
            else if (p.canon) launch_hist<16, false, 1>(ctx, p, d_codes, n_bases, k, d_hist);
            else if (p.rc) launch_hist<8, true, 0>(ctx, p, d_codes, n_bases, k, d_hist);
            else launch_hist<16, false, 0>(ctx, p, d_codes, n_bases, k, d_hist);
        } else if (p.canon && p.mix) launch_hist<12, false, 2>(ctx, p, d_codes, n_bases, k, d_hist);
        else if (p.canon) launch_hist<12, false, 1>(ctx, p, d_codes, n_bases, k, d_hist);
        else if (p.rc) launch_hist<6, true, 0>(ctx, p, d_codes, n_bases, k, d_hist);
        else launch_hist<12, false, 0>(ctx, p, d_codes, n_bases, k, d_hist);
        HIP_TRY(ctx, hipGetLastError());
    }
    HIP_TRY(ctx, hipMemcpyAsync(hist, d_hist, (size_t)RADIX * RS * 4, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return KMAN_OK;
}

extern "C" int kman_dshard_extract(kman_ctx *ctx, const uint8_t *d_codes, uint64_t n_bases, uint64_t n_bases_q,
                                   uint32_t k, uint32_t flags, int mode, const uint32_t *d_hist,
                                   const uint64_t *d_rtab, uint64_t *d_send) {
    if (!ctx) return KMAN_EINVAL;
    RegionPlan p;
    const int pr = make_shard_plan(n_bases, n_bases_q, k, flags, mode, &p);
    if (pr == KMAN_EINVAL) return kman_fail(ctx, KMAN_EINVAL, "kman_dshard_extract: bad arguments");
    if (pr != KMAN_OK) return pr;
    if (!n_bases) return KMAN_OK;
    if (!d_codes || !d_hist || !d_rtab || !d_send) return kman_fail(ctx, KMAN_EINVAL, "null buffer");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    uint32_t epoch, *counter;
    KMAN_TRY(kman_lookback_begin(ctx, 1, &epoch, &counter));  // (the XCD ticket counters only)
    {
        KTimer kt_(ctx, "region_extract");
        const uint32_t *cnt = d_hist;  // the exact region sizes (read-only)
        if (p.ei == 16 || p.ei == 8) {
            if (p.canon && p.mix) launch_extract_ex<16, false, 2>(ctx, p, d_codes, n_bases, k, d_send, cnt, d_rtab, epoch);
            else if (p.canon) launch_extract_ex<16, false, 1>(ctx, p, d_codes, n_bases, k, d_send, cnt, d_rtab, epoch);
            else if (p.rc) launch_extract_ex<8, true, 0>(ctx, p, d_codes, n_bases, k, d_send, cnt, d_rtab, epoch);
            else launch_extract_ex<16, false, 0>(ctx, p, d_codes, n_bases, k, d_send, cnt, d_rtab, epoch);
        } else if (p.canon && p.mix) launch_extract_ex<12, false, 2>(ctx, p, d_codes, n_bases, k, d_send, cnt, d_rtab, epoch);
        else if (p.canon) launch_extract_ex<12, false, 1>(ctx, p, d_codes, n_bases, k, d_send, cnt, d_rtab, epoch);
        else if (p.rc) launch_extract_ex<6, true, 0>(ctx, p, d_codes, n_bases, k, d_send, cnt, d_rtab, epoch);
        else launch_extract_ex<12, false, 0>(ctx, p, d_codes, n_bases, k, d_send, cnt, d_rtab, epoch);
        HIP_TRY(ctx, hipGetLastError());
    }
    uint32_t e;
    KMAN_TRY(read_err(ctx, &e));
    if (e) return kman_fail(ctx, KMAN_EHIP, "kman_dshard_extract: a region outgrew its rg_hist count");
    return KMAN_OK;
}

extern "C" int kman_dround_plan(uint32_t k, uint32_t flags, int mode, uint32_t world, uint64_t n_bases_q, uint32_t nb,
                                const uint64_t *counts, uint64_t *a_bytes, uint64_t *b_bytes) {
    if (!a_bytes || !b_bytes) return KMAN_EINVAL;
    *a_bytes = *b_bytes = 0;
    RoundPlan d;
    const int r = make_rplan(k, flags, mode, world, n_bases_q, nb, counts, &d);
    if (r != KMAN_OK) return r;
    *a_bytes = d.a_bytes;
    *b_bytes = d.b_bytes;
    return KMAN_OK;
}

extern "C" int kman_dround_finish(kman_ctx *ctx, const uint64_t *d_recv, uint32_t k, uint32_t flags, int mode,
                                  uint32_t world, uint64_t n_bases_q, uint32_t b_lo, uint32_t nb,
                                  const uint64_t *counts, void *d_a, uint64_t a_bytes, void *d_b, uint64_t b_bytes,
                                  uint64_t *d_okeys, void *d_ovals, uint32_t oval_bytes, uint64_t *n_out) {
    if (!ctx || !n_out) return KMAN_EINVAL;
    *n_out = 0;
    RoundPlan d;
    const int pr = make_rplan(k, flags, mode, world, n_bases_q, nb, counts, &d);
    if (pr == KMAN_EINVAL) return kman_fail(ctx, KMAN_EINVAL, "kman_dround_finish: bad arguments");
    if (pr != KMAN_OK) return pr;
    if (b_lo + nb > (uint32_t)RADIX) return kman_fail(ctx, KMAN_EINVAL, "bucket range past 256");
    if (a_bytes < d.a_bytes || b_bytes < d.b_bytes)
        return kman_fail(ctx, KMAN_ECAP, "round arenas %llu / %llu < %llu / %llu bytes", (unsigned long long)a_bytes,
                         (unsigned long long)b_bytes, (unsigned long long)d.a_bytes, (unsigned long long)d.b_bytes);
    if (oval_bytes != 4 && oval_bytes != 8) return kman_fail(ctx, KMAN_EINVAL, "oval_bytes must be 4 or 8");
    if (mode == KMAN_FINISH_UNIQ && oval_bytes != 8) return kman_fail(ctx, KMAN_EINVAL, "uniq pos on N > 1 are u64");
    if (nb == 0) return KMAN_OK;
    if (!d_recv || !d_a || !d_b || !d_okeys || !d_ovals) return kman_fail(ctx, KMAN_EINVAL, "null buffer");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    char *wa = (char *)d_a, *wb = (char *)d_b;
    uint64_t *r1 = (uint64_t *)wa;
    uint32_t *c1 = (uint32_t *)(wa + d.off_c1);
    uint64_t *sbase = (uint64_t *)(wa + d.off_tab);
    uint32_t *scnt = (uint32_t *)(sbase + (uint64_t)nb * world);
    uint64_t *r2 = (uint64_t *)wb;
    uint32_t *c2 = (uint32_t *)(wb + d.off_c2);
    uint8_t *freg = (uint8_t *)(wa + d.off_fail);
    const uint32_t G = world;
    ctx->failed.clear();
    ctx->heavy_keys = 0;
    ctx->left.valid = false;
    ctx->left.bd.clear();
    // pass-1 segments: bucket (b, src) = one contiguous run of src's chunk
    std::vector<uint64_t> hb((size_t)nb * G);
    std::vector<uint32_t> hn((size_t)nb * G);
    uint64_t roff = 0;
    for (uint32_t src = 0; src < G; src++) {
        for (uint32_t j = 0; j < nb; j++) {
            const uint64_t c = counts[(uint64_t)src * nb + j];
            hb[(size_t)j * G + src] = roff;
            hn[(size_t)j * G + src] = (uint32_t)c;
            roff += c;
        }
    }
    HIP_TRY(ctx, hipMemcpyAsync(sbase, hb.data(), hb.size() * 8, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(scnt, hn.data(), hn.size() * 4, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipMemsetAsync(c1, 0, d.nsub * 4, ctx->stream));
    HIP_TRY(ctx, hipMemsetAsync(freg, 0, d.nreg, ctx->stream));
    HeavyRound hv;
    const auto t_hv0 = std::chrono::steady_clock::now();
    {
        // (no room for the samples: the round runs without the table)
        const int hr = find_heavy(ctx, d, d_recv, hb, roff, b_lo, &hv);
        if (hr == KMAN_ENOMEM) {
            hv = HeavyRound{};
            ctx->err.clear();
            (void)hipGetLastError();
        } else if (hr != KMAN_OK) {
            return hr;
        }
    }
    const double hv_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_hv0).count();
    uint32_t epoch, *counter;
    // 4-byte count items out of pass 1 when the key bits below its digit
    // (rest + g, whatever refit_g makes of the split) fit 32 bits
    const bool narrow1 = narrow_ok(ctx, mode, d.Q, d.K - B1 - 9, 0) && !getenv("KMAN_WIDE_ITEMS");
    bool p1_lost = true;  // (no pass 1b: the finish reads pass 1's output, whose overflow loses items)
    // pass 1: by the 9 bits below the bucket, H chains per (b, src) into
    // sub-regions (b, d, src, h)
    {
        KMAN_TRY(kman_lookback_begin(ctx, 1, &epoch, &counter));
        KTimer kt_(ctx, "region_pass");
        PassArgs pa{};
        pa.in = d_recv;
        pa.seg_base = sbase;
        pa.seg_cnt = scnt;
        pa.nbk = nb * G;
        pa.nsg = 1;
        pa.gsub = G;
        pa.H = d.H;
        pa.shift = d.Q + d.K - B1 - 9;
        pa.bits = 9;
        pa.out = r1;
        pa.C1 = d.C1s;
        pa.cnt1 = c1;
        pa.fail = freg;  // sub-region (b, d, src, h) -> flag (b, d) (spread over its 2^g regions below)
        pa.fail_div = G * d.H;
        pa.fail_shift = 0;
        if (hv.n) {
            pa.hv_tab = (const uint64_t *)(hv.w + HVO_TAB);
            pa.hv_idx = (const uint32_t *)(hv.w + HVO_IDX);
            pa.hv_drop = (uint64_t *)(hv.w + HVO_DROP);
            pa.hv_q = d.Q;
            pa.hv_keep = mode == KMAN_FINISH_COUNT;
        }
        launch_pass(ctx, pa, counter, nullptr, false, narrow1);
        HIP_TRY(ctx, hipGetLastError());
    }
    KMAN_TRY(rg_check(ctx, "pass 1", c1, d.nsub));
    if (d.p1b) {
        KMAN_TRY(refit_g(ctx, d, c1, freg, G, &p1_lost));
        c2 = (uint32_t *)(wb + d.off_c2);
    }
    uint64_t *fst = nullptr;
#ifdef KMAN_RG_STAMPS
    if (getenv("KMAN_RG_STAMPS")) {
        HIP_TRY(ctx, hipMalloc((void **)&fst, d.nreg * 128));
        HIP_TRY(ctx, hipMemsetAsync(fst, 0, d.nreg * 128, ctx->stream));
    }
#endif
    if (!d.p1b) {
        // one source, two chains: the finish reads the pass-1 sub-regions
        FinishArgs f{r1, d.C1s, c1, d.Q, d.rest, (uint32_t)d.rc, (uint64_t)b_lo << 9, 0u, (uint32_t)d.nreg};
        f.fsub = d.H;
        f.freg = freg;
        f.in4 = narrow1;
        f.cap = d.cap;
        KMAN_TRY(run_finish(ctx, f, mode, d_okeys, d_ovals, oval_bytes, fst));
    } else {
    // (c2 may lie in the receive buffer: cleared only once pass 1 has read it)
    HIP_TRY(ctx, hipMemsetAsync(c2, 0, d.nreg * 4, ctx->stream));
    // pass 1b's items: 4 bytes out when the narrow finish takes them (always
    // when pass 1's were: rest <= rest + g)
    const bool narrow1b = narrow1 || (narrow_ok(ctx, mode, d.Q, d.rest, 0) && !getenv("KMAN_WIDE_ITEMS"));
    // pass 1b: per (b, d), its 2G sub-regions concatenated, by g more bits;
    // the source rank (segment index / 2) goes into the d field
    {
        KMAN_TRY(kman_lookback_begin(ctx, 1, &epoch, &counter));
        KTimer kt_(ctx, "region_pass1b");
        // count mode: a chain takes 2^m consecutive sub-buckets (their G x H
        // sub-regions lie one after another) and sorts by the g bits and the
        // low m bits of d above them -- the same regions, in the same order,
        // from fewer and longer chains (a sub-bucket alone is a few tiles,
        // whose per-chain setup and partial lines dominated); m keeps >= 1024
        // chains, <= 64 segments, <= 8 bits, and the d bits a 4-byte item holds
        // (and stops once a chain averages 64 K items: config 4's
        // sub-buckets, ~100 K each, stay one per chain)
        uint32_t m = 0;
        if (mode == KMAN_FINISH_COUNT && !getenv("KMAN_PASS1B_ONE")) {
            const uint32_t kb = d.K - B1;
            const uint64_t per_sub = roff / ((uint64_t)nb * 512);
            while (m < 5 && (per_sub << m) < 65536 && ((d.H * G) << (m + 1)) <= 64 && d.g + m + 1 <= 8 &&
                   ((nb * 512u) >> (m + 1)) >= 1024 && (!narrow1 || m + 1 + (kb - 9) <= 32))
                m++;
        }
        if (d.g == 0 && !getenv("KMAN_PASS1B_RG")) {
            // (0 bits: a merge of the sources' sub-regions, rg_merge_regions)
            const uint32_t nsg = d.H * G, tg = mode == KMAN_FINISH_UNIQ, ts = d.Q + d.rest;
            if (narrow1b != narrow1) return kman_fail(ctx, KMAN_EHIP, "pass 1b: 0-bit merge changes the item width");
            if (narrow1)
                hipLaunchKernelGGL(rg_merge_regions<uint32_t>, dim3((uint32_t)d.nreg), dim3(256), 0, ctx->stream,
                                   (const uint32_t *)r1, d.C1s, c1, nsg, d.H, (uint32_t *)r2, d.C1, c2, freg,
                                   ctx->d_err, tg, ts);
            else
                hipLaunchKernelGGL(rg_merge_regions<uint64_t>, dim3((uint32_t)d.nreg), dim3(256), 0, ctx->stream,
                                   (const uint64_t *)r1, d.C1s, c1, nsg, d.H, r2, d.C1, c2, freg, ctx->d_err, tg, ts);
            HIP_TRY(ctx, hipGetLastError());
        } else {
        PassArgs pa{};
        pa.in = r1;
        pa.seg_base = nullptr;
        pa.seg_cnt = c1;
        pa.stride = d.C1s;
        pa.nbk = (nb * 512) >> m;
        pa.nsg = (d.H * G) << m;
        pa.gsub = 1;
        pa.H = 1;
        pa.shift = d.Q + d.rest;
        pa.bits = d.g + m;
        pa.tag = mode == KMAN_FINISH_UNIQ;
        pa.tag_div = d.H;
        pa.tag_shift = d.Q + d.rest + d.g;
        pa.tag_bits = 9;
        pa.out = r2;
        pa.C1 = d.C1;
        pa.cnt1 = c2;
        pa.fail = freg;
        pa.fail_div = 1;
        pa.fail_shift = 0;
        launch_pass(ctx, pa, counter, nullptr, narrow1, narrow1b);
        HIP_TRY(ctx, hipGetLastError());
        }
    }
    KMAN_TRY(rg_check(ctx, "pass 1b", c2, d.nreg));
    if (const char *t = getenv("KMAN_TEST_LEAVE_OUT")) {
        // tests: every n-th region left out as if it had overflowed (the
        // partial redo's paths on inputs too small to overflow)
        const uint64_t every = strtoull(t, nullptr, 10);
        if (every) {
            std::vector<uint8_t> fr(d.nreg);
            HIP_TRY(ctx, hipMemcpy(fr.data(), freg, d.nreg, hipMemcpyDeviceToHost));
            for (uint64_t r = 0; r < d.nreg; r += every) fr[r] = 1;
            HIP_TRY(ctx, hipMemcpy(freg, fr.data(), d.nreg, hipMemcpyHostToDevice));
            const uint32_t ev = ERR_REGION;
            HIP_TRY(ctx, hipMemcpy(ctx->d_err, &ev, 4, hipMemcpyHostToDevice));
        }
    }
    {
        FinishArgs f{r2, d.C1, c2, d.Q, d.rest, (uint32_t)d.rc, (uint64_t)b_lo << (9 + d.g),
                     mode == KMAN_FINISH_UNIQ ? d.Q + d.rest + d.g : 0u, (uint32_t)d.nreg};
        f.freg = freg;
        f.in4 = narrow1b;
        f.cap = d.cap;
        KMAN_TRY(run_finish(ctx, f, mode, d_okeys, d_ovals, oval_bytes, fst));
    }
    }
    if (fst) KMAN_TRY(report_finish_stamps(ctx, fst, d.nreg));
    HIP_TRY(ctx, hipMemcpyAsync(ctx->h_small + 4, ctx->d_status + (d.nreg - 1), 8, hipMemcpyDeviceToHost, ctx->stream));
    uint32_t e;
    KMAN_TRY(read_err(ctx, &e));  // synchronises
    const uint64_t wd = ctx->h_small[4];
    if (((wd >> 56) & 63u) != ctx->epoch || (wd >> 62) != ST_INCL)
        return kman_fail(ctx, KMAN_EHIP, "region output total not published");
    *n_out = wd & ST_VMASK;
    ctx->heavy_keys = hv.n;
    ctx->heavy_slots = hv.slots;
    ctx->heavy_mode = mode;
    {
        // pass 1's output stays in arena A until the caller reuses it
        auto &L = ctx->left;
        L.valid = !e || (d.p1b && !p1_lost);
        L.r1 = r1;
        L.c1 = c1;
        L.C1s = d.C1s;
        L.nb = nb;
        L.G = G;
        L.H = d.H;
        L.K = d.K;
        L.Q = d.Q;
        L.b_lo = b_lo;
        L.rc = d.rc;
        L.narrow = narrow1;
        L.mode = mode;
        L.g = d.g;
        L.freg = freg;
    }
    if (hv.n && mode == KMAN_FINISH_COUNT && *n_out) {
        // the heavy keys' dropped copies onto their rows
        KTimer kt_(ctx, "heavy_fix");
        KMAN_TRY(hv_fix(ctx, hv.w, hv.slots, d_okeys, d_ovals, oval_bytes, *n_out));
        
    }
    if (!e) return KMAN_OK;
    // regions that overflowed a capacity (skewed keys: repeats) emitted
    // nothing; the rows of every other region are in place, in key order.
    // Their key ranges, merged, for the caller to redo (kman_dround_failed)
    std::vector<uint8_t> hf(d.nreg);
    HIP_TRY(ctx, hipMemcpy(hf.data(), freg, d.nreg, hipMemcpyDeviceToHost));
    const uint64_t rbase = (uint64_t)b_lo << (9 + d.g);
    const uint64_t top = d.rest >= 64 ? ~0ull : ((1ull << d.rest) - 1);
    for (uint64_t r = 0; r < d.nreg; r++) {
        if (!hf[r]) continue;
        if (ctx->left.valid && (ctx->left.bd.empty() || ctx->left.bd.back() != (uint32_t)(r >> d.g)))
            ctx->left.bd.push_back((uint32_t)(r >> d.g));
        const uint64_t lo = (rbase + r) << d.rest, hi = lo | top;
        if (!ctx->failed.empty() && ctx->failed.back() + 1 == lo) ctx->failed.back() = hi;
        else {
            ctx->failed.push_back(lo);
            ctx->failed.push_back(hi);
        }
    }
    if (getenv("KMAN_DROUND_LOG")) {
        uint64_t nf = 0;
        for (uint64_t r = 0; r < d.nreg; r++) nf += hf[r] != 0;
        fprintf(stderr, "kman_dround_finish: %llu items, nb %u G %u H %u g %u C1s %llu C1 %llu, heavy %u, pass 1 %s, "
                "%llu of %llu regions left out (%zu sub-buckets for a local redo); finding the heavy keys %.2f ms\n",
                (unsigned long long)roff, nb, G, d.H, d.g, (unsigned long long)d.C1s, (unsigned long long)d.C1, hv.n,
                p1_lost ? "lost items" : "complete", (unsigned long long)nf, (unsigned long long)d.nreg,
                ctx->left.bd.size(), hv_ms);
    }
    if (ctx->failed.empty())  // (an overflow that flagged no region: not expected)
        return kman_fail(ctx, KMAN_EHIP, "kman_dround_finish: overflow without a flagged region");
    return KMAN_EPARTIAL;
}

extern "C" int kman_dround_left(kman_ctx *ctx, uint64_t *d_keys, uint64_t *d_pos, uint64_t cap, uint64_t *n) {
    if (!ctx || !n) return KMAN_EINVAL;
    *n = 0;
    const auto &L = ctx->left;
    if (!L.valid) return KMAN_EFALLBACK;
    if (L.bd.empty()) return KMAN_OK;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const uint32_t GH = L.G * L.H;
    const uint32_t ns = (uint32_t)L.bd.size() * GH;
    std::vector<uint32_t> subs(ns);
    for (size_t i = 0; i < L.bd.size(); i++)
        for (uint32_t q = 0; q < GH; q++) subs[i * GH + q] = L.bd[i] * GH + q;
    // (the heavy-key scratch holds the sub-region list, counts and offsets)
    const size_t o_subs = HVO_END, o_cnt = o_subs + ceil_div((uint64_t)ns * 4, 256) * 256,
                 o_off = o_cnt + ceil_div((uint64_t)ns * 4, 256) * 256, bytes = o_off + (size_t)ns * 16 * 8 + 256;
    if (bytes > ctx->hv_bytes) {
        // (grows the buffer: its heavy table is copied along)
        void *nb_ = nullptr;
        if (hipMalloc(&nb_, bytes) != hipSuccess) {  // (no room: the caller's marked-extraction redo)
            (void)hipGetLastError();
            return KMAN_EFALLBACK;
        }
        if (ctx->d_hv) {
            HIP_TRY(ctx, hipMemcpyAsync(nb_, ctx->d_hv, std::min(ctx->hv_bytes, HVO_END), hipMemcpyDeviceToDevice,
                                        ctx->stream));
            HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
            HIP_TRY(ctx, hipFree(ctx->d_hv));
        }
        ctx->d_hv = nb_;
        ctx->hv_bytes = bytes;
    }
    char *w = (char *)ctx->d_hv;
    uint32_t *d_subs = (uint32_t *)(w + o_subs), *d_cnt = (uint32_t *)(w + o_cnt);
    uint64_t *d_bco = (uint64_t *)(w + o_off);  // (ns x Y <= 16 per-block counts / offsets)
    HIP_TRY(ctx, hipMemcpyAsync(d_subs, subs.data(), (size_t)ns * 4, hipMemcpyHostToDevice, ctx->stream));
    hipLaunchKernelGGL(rg_left_counts, dim3((ns + 255) / 256), dim3(256), 0, ctx->stream, L.c1, d_subs, ns, L.C1s,
                       d_cnt);
    HIP_TRY(ctx, hipGetLastError());
    std::vector<uint32_t> cnt(ns);
    HIP_TRY(ctx, hipMemcpyAsync(cnt.data(), d_cnt, (size_t)ns * 4, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    uint32_t mx = 0;
    for (uint32_t i = 0; i < ns; i++) mx = std::max(mx, cnt[i]);
    if (d_keys && L.mode == KMAN_FINISH_UNIQ && !d_pos) return kman_fail(ctx, KMAN_EINVAL, "uniq: null pos");
    KTimer kt_(ctx, "left_gather");
    const uint32_t Y = std::max<uint32_t>(1, std::min<uint32_t>(16, (mx + 2047) / 2048));
    const dim3 grid(ns, Y);
    const uint64_t nbk = (uint64_t)ns * Y;
    // the per-block counts, then (writing) their exclusive scan, in d_bco
    const auto launch = [&](bool write) {
        uint64_t *pos = write && L.mode == KMAN_FINISH_UNIQ ? d_pos : nullptr;
        uint64_t *ok = write ? d_keys : nullptr;
        if (L.narrow) {
            if (write)
                hipLaunchKernelGGL((rg_left_gather<uint32_t, true>), grid, dim3(256), 0, ctx->stream,
                                   (const uint32_t *)L.r1, L.C1s, d_subs, d_cnt, L.freg, L.g, L.G, L.H, L.b_lo,
                                   L.K - B1, L.Q, (uint32_t)L.rc, d_bco, ok, pos);
            else
                hipLaunchKernelGGL((rg_left_gather<uint32_t, false>), grid, dim3(256), 0, ctx->stream,
                                   (const uint32_t *)L.r1, L.C1s, d_subs, d_cnt, L.freg, L.g, L.G, L.H, L.b_lo,
                                   L.K - B1, L.Q, (uint32_t)L.rc, d_bco, ok, pos);
        } else {
            if (write)
                hipLaunchKernelGGL((rg_left_gather<uint64_t, true>), grid, dim3(256), 0, ctx->stream,
                                   (const uint64_t *)L.r1, L.C1s, d_subs, d_cnt, L.freg, L.g, L.G, L.H, L.b_lo,
                                   L.K - B1, L.Q, (uint32_t)L.rc, d_bco, ok, pos);
            else
                hipLaunchKernelGGL((rg_left_gather<uint64_t, false>), grid, dim3(256), 0, ctx->stream,
                                   (const uint64_t *)L.r1, L.C1s, d_subs, d_cnt, L.freg, L.g, L.G, L.H, L.b_lo,
                                   L.K - B1, L.Q, (uint32_t)L.rc, d_bco, ok, pos);
        }
        return hipGetLastError();
    };
    HIP_TRY(ctx, launch(false));
    std::vector<uint64_t> bc(nbk);
    HIP_TRY(ctx, hipMemcpyAsync(bc.data(), d_bco, nbk * 8, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    uint64_t tot = 0;
    for (uint64_t q = 0; q < nbk; q++) {
        const uint64_t c = bc[q];
        bc[q] = tot;
        tot += c;
    }
    *n = tot;
    if (!d_keys || !tot) return KMAN_OK;
    if (tot > cap)
        return kman_fail(ctx, KMAN_ECAP, "kman_dround_left: %llu items > cap %llu", (unsigned long long)tot,
                         (unsigned long long)cap);
    HIP_TRY(ctx, hipMemcpyAsync(d_bco, bc.data(), nbk * 8, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, launch(true));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));  // (bc leaves scope)
    return KMAN_OK;
}

extern "C" int kman_dround_heavy_fix(kman_ctx *ctx, const uint64_t *d_keys, void *d_vals, uint32_t val_bytes,
                                     uint64_t n) {
    if (!ctx) return KMAN_EINVAL;
    if (!ctx->heavy_keys || ctx->heavy_mode != KMAN_FINISH_COUNT || !n) return KMAN_OK;
    if (!d_keys || !d_vals) return kman_fail(ctx, KMAN_EINVAL, "null buffer");
    if (val_bytes != 4 && val_bytes != 8) return kman_fail(ctx, KMAN_EINVAL, "val_bytes must be 4 or 8");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    KMAN_TRY(hv_fix(ctx, (const char *)ctx->d_hv, ctx->heavy_slots, d_keys, d_vals, val_bytes, n));
    return KMAN_OK;
}

extern "C" int kman_dround_heavy(kman_ctx *ctx, uint32_t *n) {
    if (!ctx || !n) return KMAN_EINVAL;
    *n = ctx->heavy_keys;
    return KMAN_OK;
}

extern "C" int kman_dround_failed(kman_ctx *ctx, uint64_t *ranges, uint64_t cap, uint64_t *n) {
    if (!ctx || !n) return KMAN_EINVAL;
    *n = ctx->failed.size() / 2;
    if (!ranges) return KMAN_OK;
    if (cap < *n) return KMAN_ECAP;
    memcpy(ranges, ctx->failed.data(), ctx->failed.size() * 8);
    return KMAN_OK;
}

// ====================================================== abundance histogram
// hist[min(count, nbins - 1)] += 1 over the count output of kman_groups /
// kman_finish (COUNT): the k-mer abundance spectrum of BASELINE config 5
// (not in the reference).  hist: nbins u64, zeroed here.
namespace {
template <typename C>
__global__ __launch_bounds__(256) void count_hist_kernel(const C *__restrict__ counts, uint64_t n, uint32_t nbins,
                                                         unsigned long long *__restrict__ hist) {
    extern __shared__ uint32_t lh[];
    for (uint32_t i = threadIdx.x; i < nbins; i += 256) lh[i] = 0;
    __syncthreads();
    // counts of 1 and 2 (nearly every row of a genome's spectrum) in registers,
    // one LDS atomic per wave: every lane adding to the same LDS word
    // serialised the kernel (9.1 ms for 2.7 G rows, 1.2 TB/s).  16-byte loads,
    // four in flight per thread (one scalar load per trip ran at 1.6 TB/s)
    uint32_t r1 = 0, r2 = 0;
    auto add = [&](uint64_t c) {
        if (c == 1) r1++;
        else if (c == 2) r2++;
        else atomicAdd(&lh[c < nbins ? c : nbins - 1], 1u);
    };
    constexpr uint32_t PV = 16 / sizeof(C);  // counts per 16-byte vector
    const uint64_t nv = n / PV;
    const uint4 *v = reinterpret_cast<const uint4 *>(counts);
    const uint64_t stride = (uint64_t)gridDim.x * 256;
    uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    for (; i + 3 * stride < nv; i += 4 * stride) {
        uint4 a[4];
#pragma unroll
        for (int u = 0; u < 4; u++) a[u] = v[i + u * stride];
#pragma unroll
        for (int u = 0; u < 4; u++) {
            const C *c = reinterpret_cast<const C *>(&a[u]);
#pragma unroll
            for (uint32_t e = 0; e < PV; e++) add((uint64_t)c[e]);
        }
    }
    for (; i < nv; i += stride) {
        const uint4 a = v[i];
        const C *c = reinterpret_cast<const C *>(&a);
#pragma unroll
        for (uint32_t e = 0; e < PV; e++) add((uint64_t)c[e]);
    }
    for (uint64_t j = nv * PV + (uint64_t)blockIdx.x * 256 + threadIdx.x; j < n; j += stride) add((uint64_t)counts[j]);
    r1 = (uint32_t)__builtin_amdgcn_readlane((int)wave_inclusive_scan(r1, SumU32()), 63);
    r2 = (uint32_t)__builtin_amdgcn_readlane((int)wave_inclusive_scan(r2, SumU32()), 63);
    if ((threadIdx.x & 63) == 0) {
        if (r1) atomicAdd(&lh[1], r1);  // (nbins >= 2)
        if (r2) atomicAdd(&lh[2 < nbins ? 2 : nbins - 1], r2);
    }
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < nbins; i += 256)
        if (lh[i]) atomicAdd(&hist[i], (unsigned long long)lh[i]);
}
}  // namespace

extern "C" int kman_count_hist(kman_ctx *ctx, const void *d_counts, uint32_t count_bytes, uint64_t n,
                               uint64_t *d_hist, uint32_t nbins) {
    if (!ctx) return KMAN_EINVAL;
    if (count_bytes != 4 && count_bytes != 8) return kman_fail(ctx, KMAN_EINVAL, "count_bytes must be 4 or 8");
    if (nbins < 2 || nbins > 16384) return kman_fail(ctx, KMAN_EINVAL, "nbins must be in [2, 16384]");
    if (!d_hist || (n && !d_counts)) return kman_fail(ctx, KMAN_EINVAL, "null buffer");
    if ((uintptr_t)d_counts & 15) return kman_fail(ctx, KMAN_EINVAL, "counts must be 16-byte aligned");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipMemsetAsync(d_hist, 0, (size_t)nbins * 8, ctx->stream));
    if (n) {
        const uint64_t blocks = ceil_div(n, 256 * 64);
        const uint32_t g = (uint32_t)(blocks < 4096 ? blocks : 4096);
        KTimer kt_(ctx, "count_hist");
        if (count_bytes == 4)
            hipLaunchKernelGGL(count_hist_kernel<uint32_t>, dim3(g), dim3(256), nbins * 4, ctx->stream,
                               (const uint32_t *)d_counts, n, nbins, (unsigned long long *)d_hist);
        else
            hipLaunchKernelGGL(count_hist_kernel<uint64_t>, dim3(g), dim3(256), nbins * 4, ctx->stream,
                               (const uint64_t *)d_counts, n, nbins, (unsigned long long *)d_hist);
        HIP_TRY(ctx, hipGetLastError());
    }
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return kman_check_device_error(ctx);
}
