// runs.hip — the longest solid stretch of every record: over
// kman_window_counts' words (one u32 per base), base b is solid when its word
// is not KMAN_WC_NONE and >= min_count; a run is a maximal interval of solid
// bases inside one record; kman_record_runs writes, per record, the length of
// its longest run and the offset of the leftmost run of that length
// (`kmer screen --solid`).
//
// The start of the run that holds solid base b is
//     max(1 + the last non-solid position before b, the first base of b's record)
// The first term is a max-scan over the words alone, the second comes from the
// record table, so only the first needs a carry across tiles.  Tiles of
// RTILE = 4096 bases, 256 threads, 16 consecutive words per thread.
//
//   last_break  (pass 1) one block per tile: 1 + the position of the tile's last
//               non-solid base, 0 when every base is solid.  The tile is read
//               from its end in quarters of 1024 words (one 16-byte load per
//               thread) and the block stops at the first quarter that holds
//               one: reads end with a NONE gap, so most tiles cost one quarter.
//   scan        one block of 1024 threads: the exclusive max-scan of those
//               words over the tiles, in place, 8192 tiles per round.
//   runs        (pass 2) one block per tile.  Thread 0 cuts the slice of
//               d_rec_seq that owns the tile's bases; a slice of <= RCAP
//               entries is staged in LDS, a larger one is searched in global
//               memory (tile_records.h).  A thread turns its 16 words (four
//               16-byte loads) into a bit mask, the block max-scans the threads' last breaks (DPP
//               wave scans, one barrier), then the thread walks its 16 bases
//               and searches the slice again only where a base passes the next
//               record's first base.  At a run's end (the next base is not
//               solid, starts a record or does not exist) its length is known:
//               one 64-bit LDS atomicMax of (length << 13 | RTILE - offset of
//               its start in the tile) into the slot of its record, slot = the
//               offset of the record's first base in the tile (the record that
//               starts before the tile takes slot 0, which no other owner can
//               have).  The run that starts before the tile is the leftmost one
//               of its record there and takes the largest low field.
//               Then one thread per nonzero slot finds the record again.  A
//               record that lies inside the tile is complete: two plain
//               stores.  A record that reaches out of the tile (at most two
//               per tile: the one that starts before it, the one that ends
//               after it) writes a candidate (record, length, start) into the
//               tile's two places of the work buffer, raises len[r] with one
//               64-bit atomicMax and stores ~0 into start[r].
//   pick        one thread per candidate: where its length is len[r], one
//               64-bit atomicMin of its start into start[r].
// Integer max / min commute, every other store is the only one to its word:
// the same bytes on every call.
//
// Bounds, not values: tile_records.h for the slice; here every record index is
// checked against n_records before it addresses the output, and a record's
// first base is taken as min(entry, the base it owns), so every slot is <
// RTILE and every run start is <= its end.
//
// Algorithmic bytes: the words are read at most twice (pass 1 stops early), 8 B
// per base; 56 B of work memory per tile written and read; 16 B written per
// record.
#include "common.h"
#include "tile_records.h"

namespace {

constexpr int RT = 256;
constexpr int REI = 16;
constexpr int RTILE = RT * REI;
constexpr int RCAP = KMAN_RUNS_REC_CAP;
constexpr int RQ = RTILE / 4;   // pass 1 reads the tile in quarters
constexpr int SCAN_T = 1024;    // the scan over tiles: threads,
constexpr int SCAN_E = 8;       // tiles per thread and round
constexpr uint32_t BEFORE = RTILE + 1;  // low key field of the run that starts before the tile
constexpr uint64_t WORK_PER_TILE = 56;  // one scan word and two candidates of three words
static_assert(RTILE == KMAN_RUNS_TILE, "include/kman.h states the tile size");
static_assert(RQ == RT * 4, "one 16-byte load per thread and quarter");
static_assert(BEFORE < (1u << 13), "the low key field has 13 bits");

#define WC_NONE KMAN_WC_NONE

KMAN_DEV bool is_solid(uint32_t w, uint32_t min_count) { return w != WC_NONE && w >= min_count; }

// pass 1: agg[t] = 1 + the position of tile t's last non-solid base, 0 when it has none
__global__ __launch_bounds__(RT) void runs_last_break_kernel(const uint32_t *__restrict__ wc, uint64_t n_bases,
                                                             uint32_t min_count, uint64_t *__restrict__ agg) {
    __shared__ uint32_t s_m;
    const uint64_t tb = (uint64_t)blockIdx.x * RTILE;
    if (threadIdx.x == 0) s_m = 0;
    __syncthreads();
    for (int c = RTILE / RQ - 1; c >= 0; c--) {
        const uint32_t o = (uint32_t)c * RQ + threadIdx.x * 4;
        const uint64_t b = tb + o;
        uint32_t w[4] = {0, 0, 0, 0};
        if (b + 4 <= n_bases) {
            const uint4 v = *reinterpret_cast<const uint4 *>(wc + b);
            w[0] = v.x, w[1] = v.y, w[2] = v.z, w[3] = v.w;
        } else {
#pragma unroll
            for (int j = 0; j < 4; j++) w[j] = b + j < n_bases ? wc[b + j] : min_count;  // (past the end: no break)
        }
        uint32_t m = 0;
#pragma unroll
        for (int j = 0; j < 4; j++)
            if (!is_solid(w[j], min_count)) m = o + j + 1;
        if (m) atomicMax(&s_m, m);
        if (__syncthreads_or(m != 0)) break;  // (block-uniform; the barrier orders the atomics before the read below)
    }
    if (threadIdx.x == 0) agg[blockIdx.x] = s_m ? tb + s_m : 0;
}

// agg[t] <- max(agg[0 .. t)), in place; one block
__global__ __launch_bounds__(SCAN_T) void runs_scan_kernel(uint64_t *__restrict__ agg, uint64_t tiles) {
    __shared__ uint64_t lds[SCAN_T / 64];
    const uint64_t per = (uint64_t)SCAN_T * SCAN_E;
    const uint64_t rounds = (tiles + per - 1) / per;
    uint64_t carry = 0;
    for (uint64_t it = 0; it < rounds; it++) {
        const uint64_t base = it * per + (uint64_t)threadIdx.x * SCAN_E;
        uint64_t v[SCAN_E], mine = 0;
#pragma unroll
        for (int q = 0; q < SCAN_E; q++) {
            v[q] = base + q < tiles ? agg[base + q] : 0;
            mine = umax64(mine, v[q]);
        }
        uint64_t total = 0;
        const uint64_t ex = block_exclusive_scan<SCAN_T>(mine, MaxU64(), (uint64_t)0, lds, &total);
        uint64_t run = umax64(carry, ex);
#pragma unroll
        for (int q = 0; q < SCAN_E; q++) {
            if (base + q < tiles) agg[base + q] = run;
            run = umax64(run, v[q]);
        }
        carry = umax64(carry, total);
    }
}

// pass 2
__global__ __launch_bounds__(RT) void runs_kernel(const uint32_t *__restrict__ wc, uint64_t n_bases,
                                                  const uint64_t *__restrict__ rec_seq, uint64_t n_records,
                                                  uint32_t min_count, const uint64_t *__restrict__ carry_of,
                                                  uint64_t *__restrict__ cand, unsigned long long *__restrict__ out) {
    __shared__ __attribute__((aligned(16))) unsigned long long skey[RTILE];
    __shared__ uint64_t srec[RCAP + 1];
    __shared__ uint32_t s_scan[RT / 64];
    __shared__ uint8_t s_first[RT];
    __shared__ uint64_t s_r0, s_ns, s_next;

    const uint64_t tb = (uint64_t)blockIdx.x * RTILE;
    const uint64_t tend = umin64(tb + RTILE, n_bases);  // (tb < n_bases: the grid is ceil(n_bases / RTILE))
    if (threadIdx.x == 0) {
        const TileSlice s = cut_slice(rec_seq, n_records, tb, tend - 1, n_bases);  // the records that own [tb, tend)
        s_r0 = s.r0;
        s_ns = s.ns;
        s_next = s.next;
    }
    // the thread's 16 words as a mask of solid bases (past n_bases: not solid)
    const uint64_t p0 = tb + (uint64_t)threadIdx.x * REI;
    uint32_t m = 0;
    if (p0 + REI <= n_bases) {
        const uint4 *src = reinterpret_cast<const uint4 *>(wc + p0);
#pragma unroll
        for (int q = 0; q < REI / 4; q++) {
            const uint4 v = src[q];
            m |= (uint32_t)is_solid(v.x, min_count) << (4 * q);
            m |= (uint32_t)is_solid(v.y, min_count) << (4 * q + 1);
            m |= (uint32_t)is_solid(v.z, min_count) << (4 * q + 2);
            m |= (uint32_t)is_solid(v.w, min_count) << (4 * q + 3);
        }
    } else {
#pragma unroll
        for (int j = 0; j < REI; j++)
            if (p0 + j < n_bases) m |= (uint32_t)is_solid(wc[p0 + j], min_count) << j;
    }
    // the first base after the tile (thread RT - 1's right neighbour)
    bool after_solid = false;
    if (threadIdx.x == RT - 1 && tb + RTILE < n_bases) after_solid = is_solid(wc[tb + RTILE], min_count);
    const uint64_t carry = carry_of[blockIdx.x];
    __syncthreads();
    const uint64_t r0 = s_r0, ns = s_ns, next = s_next;
    if (ns == 0) return;  // (no record starts at or before the tile's last base)
    const SliceView sv = stage_slice<RT, RCAP, TAIL_NEXT>(rec_seq, {r0, ns, next}, srec);
    for (uint32_t i = threadIdx.x; i < (uint32_t)(RTILE / 2); i += RT)
        reinterpret_cast<uint4 *>(skey)[i] = make_uint4(0, 0, 0, 0);
    s_first[threadIdx.x] = (uint8_t)(m & 1u);
    // 1 + the tile offset of the thread's last non-solid base; max-scanned over the threads
    const uint32_t nm = ~m & 0xFFFFu;
    const uint32_t mine = nm ? threadIdx.x * REI + (32u - (uint32_t)__clz((int)nm)) : 0u;
    const uint32_t ex = block_exclusive_scan1<RT>(mine, MaxU32(), 0u, s_scan, (uint32_t *)nullptr);
    // (the barrier inside the scan: srec, skey and s_first are written)

    const uint64_t *rs = sv.rs;

    if (m) {
        const bool right_solid = threadIdx.x == RT - 1 ? after_solid : (s_first[threadIdx.x + 1] != 0);
        uint64_t brk = ex ? tb + ex : carry;  // 1 + the last non-solid position so far
        uint64_t u = upper_count(rs, ns, p0);
        bool owned = u != 0;                                   // (false: bases before the first record)
        uint64_t cur = owned ? umin64(rs[u - 1], p0) : p0;     // the first base of the current record
        uint64_t nxt = sv.ent(u);                                 // the base where the owner changes
#pragma unroll
        for (int j = 0; j < REI; j++) {
            const uint64_t b = p0 + j;
            if (b >= n_bases) break;
            if (j != 0 && b >= nxt) {
                u = upper_count(rs, ns, b);
                owned = u != 0;
                cur = b;
                nxt = sv.ent(u);
            }
            if (!((m >> j) & 1u)) {
                brk = b + 1;
                continue;
            }
            const bool more = j + 1 < REI ? ((m >> (j + 1)) & 1u) != 0 : right_solid;
            if ((more && b + 1 < nxt) || !owned) continue;  // not a run's end, or nobody's
            const uint64_t start = umax64(brk, cur);         // (brk <= b and cur <= b)
            const uint64_t len = b + 1 - start;
            const uint32_t slot = cur > tb ? (uint32_t)(cur - tb) : 0u;             // (cur <= b: < RTILE)
            const uint32_t field = start >= tb ? (uint32_t)RTILE - (uint32_t)(start - tb) : BEFORE;
            if (slot < (uint32_t)RTILE)
                atomicMax(&skey[slot], (unsigned long long)((len << 13) | (uint64_t)field));
        }
    }
    __syncthreads();

    for (uint32_t i = threadIdx.x; i < (uint32_t)RTILE; i += RT) {
        const uint64_t key = skey[i];
        if (key == 0) continue;
        const uint64_t u = upper_count(rs, ns, tb + i);
        if (u == 0) continue;  // (cannot happen: the slot's base has an owner)
        const uint64_t r = r0 + (u - 1);
        if (r >= n_records) continue;  // (cannot happen: u <= ns and r0 + ns <= n_records)
        const uint64_t s = umin64(rs[u - 1], tb + i);
        const uint64_t e = umin64(sv.ent(u), n_bases);
        const uint64_t len = key >> 13;
        const uint32_t field = (uint32_t)(key & 8191u);
        const uint64_t start = field == BEFORE ? umax64(carry, s) : tb + ((uint64_t)RTILE - field);
        const uint64_t off = start - s;
        if (s >= tb && e <= tend) {
            // the whole record lies in this tile: its only writer
            out[r] = off;
            out[n_records + r] = len;
        } else {
            uint64_t *c = cand + 6 * (uint64_t)blockIdx.x + (s < tb ? 0 : 3);
            c[0] = r;
            c[1] = len;
            c[2] = off;
            atomicMax(&out[n_records + r], (unsigned long long)len);
            out[r] = ~0ull;  // (every writer stores this; runs_pick_kernel lowers it)
        }
    }
}

// one thread per candidate: the leftmost start among those of the record's best length
__global__ __launch_bounds__(256) void runs_pick_kernel(const uint64_t *__restrict__ cand, uint64_t n_cand,
                                                        uint64_t n_records, unsigned long long *__restrict__ out) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n_cand) return;
    const uint64_t r = cand[3 * i], len = cand[3 * i + 1], off = cand[3 * i + 2];
    if (len == 0 || r >= n_records) return;
    if (out[n_records + r] == len) atomicMin(&out[r], (unsigned long long)off);
}

uint64_t work_of(uint64_t tiles) {
    const uint64_t b = WORK_PER_TILE * tiles;
    return b < 16 ? 16 : (b + 15) & ~15ull;
}

}  // namespace

extern "C" int kman_record_runs_plan(uint64_t n_bases, uint64_t n_records, uint64_t *work_bytes) {
    if (!work_bytes) return KMAN_EINVAL;
    *work_bytes = 0;
    const uint64_t tiles = n_bases / RTILE + (n_bases % RTILE != 0);
    if (tiles > 0x7ffffffeull || n_records > (~0ull >> 5)) return KMAN_EINVAL;
    *work_bytes = work_of(tiles);
    return KMAN_OK;
}

extern "C" int kman_record_runs(kman_ctx *ctx, const void *d_wc, uint64_t n_bases, const void *d_rec_seq,
                                uint64_t n_records, uint32_t min_count, void *d_work, uint64_t work_bytes,
                                void *d_out) {
    if (!ctx) return KMAN_EINVAL;
    if (min_count < 1 || min_count > 0xFFFFFFFEu)
        return kman_fail(ctx, KMAN_EINVAL, "min_count must be in [1, 4294967294], got %u", min_count);
    if (n_records == 0) return KMAN_OK;
    if (!d_rec_seq || !d_out || (n_bases && (!d_wc || !d_work)))
        return kman_fail(ctx, KMAN_EINVAL, "kman_record_runs: null buffer");
    if (((uintptr_t)d_wc & 15) != 0 || ((uintptr_t)d_work & 15) != 0)
        return kman_fail(ctx, KMAN_EINVAL, "d_wc and d_work must be 16-byte aligned");
    uint64_t want = 0;
    if (kman_record_runs_plan(n_bases, n_records, &want) != KMAN_OK)
        return kman_fail(ctx, KMAN_EINVAL, "%llu bases, %llu records: too many", (unsigned long long)n_bases,
                         (unsigned long long)n_records);
    if (n_bases && work_bytes < want)
        return kman_fail(ctx, KMAN_ECAP, "work buffer of %llu bytes: kman_record_runs_plan asks for %llu",
                         (unsigned long long)work_bytes, (unsigned long long)want);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipMemsetAsync(d_out, 0, (size_t)(16 * n_records), ctx->stream));
    if (n_bases) {
        const uint64_t tiles = ceil_div(n_bases, RTILE);
        uint64_t *d_agg = (uint64_t *)d_work, *d_cand = d_agg + tiles;
        HIP_TRY(ctx, hipMemsetAsync(d_cand, 0, (size_t)(48 * tiles), ctx->stream));
        KTimer kt_(ctx, "record_runs");
        hipLaunchKernelGGL(runs_last_break_kernel, dim3((uint32_t)tiles), dim3(RT), 0, ctx->stream,
                           (const uint32_t *)d_wc, n_bases, min_count, d_agg);
        HIP_TRY(ctx, hipGetLastError());
        hipLaunchKernelGGL(runs_scan_kernel, dim3(1), dim3(SCAN_T), 0, ctx->stream, d_agg, tiles);
        HIP_TRY(ctx, hipGetLastError());
        hipLaunchKernelGGL(runs_kernel, dim3((uint32_t)tiles), dim3(RT), 0, ctx->stream, (const uint32_t *)d_wc,
                           n_bases, (const uint64_t *)d_rec_seq, n_records, min_count, d_agg, d_cand,
                           (unsigned long long *)d_out);
        HIP_TRY(ctx, hipGetLastError());
        hipLaunchKernelGGL(runs_pick_kernel, dim3((uint32_t)ceil_div(2 * tiles, 256)), dim3(256), 0, ctx->stream,
                           d_cand, 2 * tiles, n_records, (unsigned long long *)d_out);
        HIP_TRY(ctx, hipGetLastError());
    }
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return KMAN_OK;
}
