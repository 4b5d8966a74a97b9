// region_pass.hip — the digit passes of the region path (region.h): rg_pass
// (pass 1, and pass 1b of the key rounds) and rg_merge_regions (pass 1b with 0
// bits).  PassArgs, the input of a pass, is described in region.h.
#include "region.h"

using namespace kman::region;

namespace {

// ---------------------------------------------------------------- pass 1
constexpr int R1 = 512;  // pass-1 radix bound

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
template <typename TI, typename TO, int NT_ = PT_NT, int RB = R1, bool LN = false, bool HV = false>
__global__ __launch_bounds__(NT_, 4) void rg_pass(PassArgs pa, uint32_t *__restrict__ counter,
                                                 uint32_t *__restrict__ err, uint64_t *__restrict__ stp) {
    constexpr int NT = NT_, SI = HV ? PT_SI - 1 : PT_SI, TILE = NT * SI, NWAVE = NT / 64;  // (HV: 7 items, no spills)
    static_assert(!LN || (!HV && sizeof(TI) == 8 && sizeof(TO) == 8 && NT == 1024 && RB == 512),
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
#pragma unroll
            for (int i = 0; i < SI; i++) rank[i] = (vm >> i) & 1u ? atomicAdd(&thist[PDIGIT(key[i])], 1u) : 0u;
            __syncthreads();
            if constexpr (LN) {
                // digit d's ring: its 2^lb lines, RING items; stream line g
                // (items [32 g, 32 g + 32) of d's sub-region) sits in line
                // (d << lb) | (g & lm); the first line not yet stored is run[d] >> 5
                // (line1, a test setting: one line per digit at any width)
                const uint32_t lb = pa.line1 ? 0u : 9u - bits, lm = (1u << lb) - 1, RING = 32u << lb;
                if (threadIdx.x < RB) {
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
    // radix <= 256: the 512-thread instance, two blocks per CU
    if (pa.bits <= 8 && !pa.big) {
        const uint32_t grid = (uint32_t)kman_persistent_grid(ctx, (const void *)rg_pass<TI, TO, 512, 256>, 512,
                                                             (uint64_t)pa.nbk * pa.H);
        hipLaunchKernelGGL((rg_pass<TI, TO, 512, 256>), dim3(grid), dim3(512), 0, ctx->stream, pa, counter,
                           ctx->d_err, stp);
        return;
    }
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
    const uint32_t grid =
        (uint32_t)kman_persistent_grid(ctx, (const void *)rg_pass<TI, TO>, PT_NT, (uint64_t)pa.nbk * pa.H);
    hipLaunchKernelGGL((rg_pass<TI, TO>), dim3(grid), dim3(PT_NT), 0, ctx->stream, pa, counter, ctx->d_err, stp);
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

}  // namespace

int kman::region::launch_pass(kman_ctx *ctx, const PassArgs &pa, uint32_t *counter, uint64_t *stp, bool in4,
                              bool out4) {
    // (a pass 1b of 0 bits is a merge: launch_merge_regions)
    if (pa.bits == 0) return kman_fail(ctx, KMAN_EINVAL, "launch_pass: a digit pass of 0 bits");
    if (in4) launch_pass_as<uint32_t, uint32_t>(ctx, pa, counter, stp);
    else if (out4) launch_pass_as<uint64_t, uint32_t>(ctx, pa, counter, stp);
    else launch_pass_as<uint64_t, uint64_t>(ctx, pa, counter, stp);
    return KMAN_OK;
}

int kman::region::launch_merge_regions(kman_ctx *ctx, bool narrow, const void *in, uint64_t C1s, const uint32_t *c1,
                                       uint32_t nsg, uint32_t H, void *out, uint64_t C1, uint32_t *c2, uint8_t *freg,
                                       uint32_t nreg, uint32_t tag, uint32_t tag_shift) {
    if (narrow)
        hipLaunchKernelGGL(rg_merge_regions<uint32_t>, dim3(nreg), dim3(256), 0, ctx->stream, (const uint32_t *)in,
                           C1s, c1, nsg, H, (uint32_t *)out, C1, c2, freg, ctx->d_err, tag, tag_shift);
    else
        hipLaunchKernelGGL(rg_merge_regions<uint64_t>, dim3(nreg), dim3(256), 0, ctx->stream, (const uint64_t *)in,
                           C1s, c1, nsg, H, (uint64_t *)out, C1, c2, freg, ctx->d_err, tag, tag_shift);
    HIP_TRY(ctx, hipGetLastError());
    return KMAN_OK;
}
