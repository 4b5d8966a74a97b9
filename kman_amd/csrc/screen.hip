// screen.hip — reads against a table: for every record, how many of its
// k-mer windows are rows of a count table, and the sum of those rows' counts.
//
// kman_table_index builds a prefix index over a table of strictly ascending
// keys: d_index[p] = the number of rows whose top index_bits key bits are < p,
// so bucket p is rows [d_index[p], d_index[p + 1]).  One thread per entry, a
// lower bound over the keys in bits(nt) <= 64 steps.
//
// kman_screen_records, one block of 256 threads per tile of STILE = 4096
// windows (extract_kernel's tile: stage_codes + roll<16, CANON>):
//   lookup     a thread's 16 windows advance in lockstep: the 16 index pairs
//              are loaded, then step 1 of all 16 searches, then step 2, ..: 16
//              independent loads in flight per thread, not 16 dependent chains
//              one after another.  A search halves its bucket; the step count
//              is bits(largest bucket of the thread) <= 64.  A probe that reads
//              the key itself marks the hit (a lower bound that ends inside
//              the bucket has probed the row it ends on), so a bucket of n
//              rows costs floor(log2 n) + 1 key reads, and a hit one count read.
//   records    thread 0 cuts the slice of d_rec_seq that owns the tile's bases;
//              a slice of <= SCAP entries is staged in LDS, a larger one is
//              searched in global memory; a thread walks its 16 consecutive
//              windows by runs of one record (tile_records.h: cut_slice,
//              stage_slice, owner_walk).
//   reduction  runs of one record are added to LDS slots (windows, hits: u32;
//              count sum: u64), then each nonzero (slot, plane) is one 64-bit
//              atomicAdd to d_out.  LDS path: slot = record - first record of
//              the slice, one round.  Global path: slot = the offset of the
//              record's first base in the tile (every record that owns a base
//              of the tile starts at its own offset; the one that starts
//              before the tile takes offset 0, which no other owner can have),
//              in STILE / SCAP rounds of SCAP offsets.  Integer adds commute:
//              the result does not depend on the order of the atomics.
//
// Bounds, not values: tile_records.h for the records and slots, screen_lookup.h
// for the table; here every record that addresses d_out is checked against
// n_records.
//
// Algorithmic bytes per valid window: 1 B code, one 16 B index pair, at most
// floor(log2 bucket) + 1 random 8 B key reads (each a 64 B sector or more from
// HBM when the table is larger than the caches), 4 / 8 B of count on a hit.
#include "common.h"
#include "kmer.h"
#include "screen_lookup.h"
#include "tile_records.h"

namespace {

constexpr int ST = 256;
constexpr int SEI = 16;
constexpr int STILE = ST * SEI;
constexpr int SCAP = KMAN_SCREEN_REC_CAP;
static_assert(STILE == KMAN_SCREEN_TILE, "include/kman.h states the tile size");
static_assert(STILE % SCAP == 0, "the global path's rounds tile the offsets");

inline uint32_t host_steps_of(uint64_t len) {
    uint32_t s = 0;
    for (; len; len >>= 1) s++;
    return s;
}

__global__ __launch_bounds__(256) void table_index_kernel(const uint64_t *__restrict__ tkeys, uint64_t nt,
                                                          uint32_t shift, uint32_t index_bits, uint32_t nsteps,
                                                          uint64_t *__restrict__ index) {
    const uint64_t p = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    const uint64_t np = 1ull << index_bits;
    if (p > np) return;
    uint64_t lo = 0, len = p == np ? 0 : nt;  // (the last entry is nt itself: 2^index_bits << shift may be 2^64)
    if (p == np) lo = nt;
    const uint64_t x = p << shift;  // the first row with key >= x
    for (uint32_t s = 0; s < nsteps; s++) {
        const uint64_t half = len >> 1;
        if (len != 0 && tkeys[lo + half] < x) {
            lo += half + 1;
            len -= half + 1;
        } else {
            len = half;
        }
    }
    index[p] = lo;
}

template <int CANON, typename CT>
__global__ __launch_bounds__(ST) void screen_kernel(const uint8_t *__restrict__ codes, uint64_t n_bases, int k,
                                                    const uint64_t *__restrict__ rec_seq, uint64_t n_records,
                                                    const uint64_t *__restrict__ tkeys, const CT *__restrict__ tcounts,
                                                    uint64_t nt, const uint64_t *__restrict__ index, uint32_t shift,
                                                    unsigned long long *__restrict__ out) {
    __shared__ __attribute__((aligned(16))) uint8_t scodes[STILE + 64];
    __shared__ uint64_t srec[SCAP];  // LDS path: the slice of rec_seq; global path: the record of each slot
    __shared__ uint32_t sw[SCAP], sh[SCAP];
    __shared__ unsigned long long ss[SCAP];
    __shared__ uint64_t s_r0, s_ns;

    const uint64_t tb = (uint64_t)blockIdx.x * STILE;
    if (threadIdx.x == 0) {
        // the records that own bases [tb, last]: from the owner of tb (or the
        // first record, when none starts at or before tb) to the owner of last
        const TileSlice s = cut_slice(rec_seq, n_records, tb, umin64(tb + STILE, n_bases) - 1);
        s_r0 = s.r0;
        s_ns = s.ns;
    }
    stage_codes<ST, SEI>(codes, n_bases, tb, scodes);
    __syncthreads();
    const uint64_t r0 = s_r0, ns = s_ns;
    if (ns == 0) return;  // (no record starts at or before the tile's last base)
    const SliceView sv = stage_slice<ST, SCAP>(rec_seq, {r0, ns, 0}, srec);
    const bool big = sv.big;

    const uint64_t mask = k == 32 ? ~0ull : ((1ull << (2 * k)) - 1);
    uint64_t kf[SEI], kr[SEI];
    const uint64_t p0 = tb + (uint64_t)threadIdx.x * SEI;
    const uint32_t valid = roll<SEI, CANON>(scodes, threadIdx.x * SEI, k, mask, p0, n_bases, kf, kr);

    // ---- lookup: 16 searches in lockstep (screen_lookup.h, shared with kman_window_counts)
    uint64_t cnt[SEI];
    const uint32_t hit = table_lookup<SEI, CT>(valid, kf, shift, index, tkeys, tcounts, nt, cnt);

    // ---- per-record reduction
    struct Run {
        uint32_t h;
        uint64_t sum;
    };
    const int rounds = big ? STILE / SCAP : 1;
    for (int c = 0; c < rounds; c++) {
        for (uint32_t i = threadIdx.x; i < (uint32_t)SCAP; i += ST) {
            sw[i] = 0;
            sh[i] = 0;
            ss[i] = 0;
        }
        __syncthreads();  // (and, in round 0, the slice in srec)
        if (valid)
            owner_walk<SEI, SCAP, Run>(
                sv, r0, tb, p0, valid, c, srec,
                [&](Run &a, int j) {
                    a.h += (hit >> j) & 1u;
                    a.sum += cnt[j];
                },
                [&](const Run &a, uint32_t w, uint32_t slot) {
                    atomicAdd(&sw[slot], w);
                    if (a.h) atomicAdd(&sh[slot], a.h);
                    if (a.sum) atomicAdd(&ss[slot], (unsigned long long)a.sum);
                });
        __syncthreads();
        for (uint32_t i = threadIdx.x; i < (uint32_t)SCAP; i += ST) {
            const uint32_t wv = sw[i];
            if (wv == 0) continue;
            const uint64_t r = big ? srec[i] : r0 + i;
            if (r >= n_records) continue;  // (cannot happen: r < r0 + ns <= n_records)
            atomicAdd(&out[r], (unsigned long long)wv);
            if (sh[i]) atomicAdd(&out[n_records + r], (unsigned long long)sh[i]);
            if (ss[i]) atomicAdd(&out[2 * n_records + r], ss[i]);
        }
        __syncthreads();
    }
}

template <int CANON, typename CT>
void launch_screen(kman_ctx *ctx, const uint8_t *codes, uint64_t n_bases, uint32_t k, const uint64_t *rec_seq,
                   uint64_t n_records, const uint64_t *tkeys, const void *tcounts, uint64_t nt, const uint64_t *index,
                   uint32_t shift, uint64_t *out, uint64_t tiles) {
    hipLaunchKernelGGL((screen_kernel<CANON, CT>), dim3((uint32_t)tiles), dim3(ST), 0, ctx->stream, codes, n_bases,
                       (int)k, rec_seq, n_records, tkeys, (const CT *)tcounts, nt, index, shift,
                       (unsigned long long *)out);
}

}  // namespace

extern "C" int kman_table_index(kman_ctx *ctx, const uint64_t *d_tkeys, uint64_t nt, uint32_t k, uint32_t index_bits,
                                uint64_t *d_index) {
    if (!ctx) return KMAN_EINVAL;
    if (k < 2 || k > 32) return kman_fail(ctx, KMAN_EINVAL, "k must be in [2, 32] on the GPU path, got %u", k);
    if (!index_bits_ok(k, index_bits))
        return kman_fail(ctx, KMAN_EINVAL, "index_bits must be in [1, min(2k, %d)], got %u (k = %u)",
                         KMAN_SCREEN_MAX_INDEX_BITS, index_bits, k);
    if (!d_index || (nt && !d_tkeys)) return kman_fail(ctx, KMAN_EINVAL, "kman_table_index: null buffer");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const uint64_t entries = (1ull << index_bits) + 1;
    {
        KTimer kt_(ctx, "table_index");
        hipLaunchKernelGGL(table_index_kernel, dim3((uint32_t)ceil_div(entries, 256)), dim3(256), 0, ctx->stream,
                           d_tkeys, nt, 2 * k - index_bits, index_bits, host_steps_of(nt), d_index);
        HIP_TRY(ctx, hipGetLastError());
    }
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return KMAN_OK;
}

extern "C" int kman_screen_records(kman_ctx *ctx, const uint8_t *d_codes, uint64_t n_bases, uint32_t k, uint32_t flags,
                                   const uint64_t *d_rec_seq, uint64_t n_records, const uint64_t *d_tkeys,
                                   const void *d_tcounts, uint32_t t_count_bytes, uint64_t nt, const uint64_t *d_index,
                                   uint32_t index_bits, uint64_t *d_out) {
    if (!ctx) return KMAN_EINVAL;
    if (k < 2 || k > 32) return kman_fail(ctx, KMAN_EINVAL, "k must be in [2, 32] on the GPU path, got %u", k);
    if (flags & ~KMAN_CANONICAL) return kman_fail(ctx, KMAN_EINVAL, "kman_screen_records: flags 0x%x", flags);
    if (t_count_bytes != 4 && t_count_bytes != 8)
        return kman_fail(ctx, KMAN_EINVAL, "count widths must be 4 or 8 bytes");
    if (!index_bits_ok(k, index_bits))
        return kman_fail(ctx, KMAN_EINVAL, "index_bits must be in [1, min(2k, %d)], got %u (k = %u)",
                         KMAN_SCREEN_MAX_INDEX_BITS, index_bits, k);
    if (n_records == 0) return KMAN_OK;
    if (!d_out || !d_rec_seq) return kman_fail(ctx, KMAN_EINVAL, "kman_screen_records: null buffer");
    if (n_records > (~0ull >> 2) / 8) return kman_fail(ctx, KMAN_EINVAL, "too many records");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipMemsetAsync(d_out, 0, (size_t)(24 * n_records), ctx->stream));
    if (n_bases >= k) {
        if (!d_codes || !d_index || (nt && (!d_tkeys || !d_tcounts)))
            return kman_fail(ctx, KMAN_EINVAL, "kman_screen_records: null buffer");
        if (((uintptr_t)d_codes & 15) != 0) return kman_fail(ctx, KMAN_EINVAL, "codes must be 16-byte aligned");
        const uint64_t tiles = ceil_div(n_bases, STILE);
        if (tiles > 0x7ffffffeull)
            return kman_fail(ctx, KMAN_EINVAL, "%llu bases: too many tiles", (unsigned long long)n_bases);
        const uint32_t shift = 2 * k - index_bits;
        KTimer kt_(ctx, "screen");
        if (flags & KMAN_CANONICAL) {
            if (t_count_bytes == 4)
                launch_screen<1, uint32_t>(ctx, d_codes, n_bases, k, d_rec_seq, n_records, d_tkeys, d_tcounts, nt,
                                           d_index, shift, d_out, tiles);
            else
                launch_screen<1, uint64_t>(ctx, d_codes, n_bases, k, d_rec_seq, n_records, d_tkeys, d_tcounts, nt,
                                           d_index, shift, d_out, tiles);
        } else {
            if (t_count_bytes == 4)
                launch_screen<0, uint32_t>(ctx, d_codes, n_bases, k, d_rec_seq, n_records, d_tkeys, d_tcounts, nt,
                                           d_index, shift, d_out, tiles);
            else
                launch_screen<0, uint64_t>(ctx, d_codes, n_bases, k, d_rec_seq, n_records, d_tkeys, d_tcounts, nt,
                                           d_index, shift, d_out, tiles);
        }
        HIP_TRY(ctx, hipGetLastError());
    }
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return KMAN_OK;
}
