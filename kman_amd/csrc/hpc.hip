// hpc.hip — homopolymer compression of the parsed codes (`--hpc`): every run
// of one base collapses to its first base before k-mers are taken, so a wrong
// homopolymer length (the dominant error of long reads) no longer costs up to
// k windows.  A segmented stream compaction over one byte per base.
//
// The rule (include/kman.h): base i is dropped exactly when i > 0, bits 2 and
// 3 of code[i] are clear and (code[i - 1] & 7) == (code[i] & 7).  Bit 3 opens a
// record, so no run crosses a record boundary; bit 2 (N, other letters, a -q
// mask) is never dropped and never equals an ACGT code in its low three bits.
//
//   compact  one block per KMAN_HPC_TILE input bytes (256 threads x 2 x 16 B).
//            Wave w owns the tile's bytes [2048 w, 2048 w + 2048); lane l's
//            word j is the 16 bytes from (64 j + l) * 16 there, so a load of
//            the wave reads one contiguous KiB and the rank order (wave, j,
//            lane, byte) is the input order.  The byte before a word comes
//            from the lane below (DPP), from lane 63 of the word group below,
//            or, for the wave's first byte, from d_codes.  Keep flags are
//            byte-parallel arithmetic on the four dwords; the counts of the
//            two words are ranked with one packed DPP wave scan; the tile's
//            output offset is the decoupled look-back of common.h (dynamic
//            tile ids).  The kept bytes go to LDS at (offset % 16) + rank, so
//            LDS and d_out_codes agree mod 16, and leave as aligned 16-byte
//            words; the first and last word of a tile's range, which it may
//            share with its neighbours, are written byte by byte: every
//            output byte has one writer.  With d_orig the kept bytes'
//            tile-local offsets are staged beside them (u16) and leave as
//            coalesced u64.  Lanes 0, 16, 32, 48 note the kept bytes before
//            their word in d_grp: one prefix per KMAN_HPC_GROUP input bytes.
//   table    one thread per record: the prefix of the group that holds the
//            record's first base plus the kept bytes from the group's start to
//            that base, at most KMAN_HPC_GROUP / 16 words, flags by the same
//            function.  A record that starts at n_bases gets the total.
//
// Algorithmic bytes: n_bases read, the kept bytes written, 8 B per kept base
// with d_orig; 8 B of prefix per 256 input bytes written, 16 B per record for
// the tables plus its group's bytes (cached) read.
//
// Bounds, not values: a table entry is clamped to n_bases; an input byte is
// read only below n_bases; an output byte is written only below the tile's
// offset plus its kept count, at most n_bases; both record loops run a step
// count fixed before they start.
#include "bytes16.h"
#include "common.h"

namespace {

constexpr int HT = 256;                   // threads per tile
constexpr int HG = 2;                     // 16-byte words per thread
constexpr int HWAVE = 64 * HG * 16;       // consecutive bytes of one wave
constexpr int HTILE = (HT / 64) * HWAVE;  // bytes per tile
constexpr int GROUP = KMAN_HPC_GROUP;
static_assert(HTILE == KMAN_HPC_TILE, "include/kman.h states the tile size");
static_assert(GROUP == 16 * 16, "sixteen lanes' words make a prefix group");

// the four bytes of w that are KEPT, as bits 0-3; prev: the byte before w's first
KMAN_DEV uint32_t keep4(uint32_t w, uint32_t prev) {
    const uint32_t pw = (w << 8) | (prev & 0xffu);
    // a byte of y is 0 exactly when the code equals its predecessor in bits 0-2 and has bits 2, 3 clear
    const uint32_t y = ((w ^ pw) & 0x07070707u) | (w & 0x0c0c0c0cu);
    const uint32_t t = (y | (y >> 1) | (y >> 2) | (y >> 3)) & 0x01010101u;  // (a byte of y is < 16)
    return (t | (t >> 7) | (t >> 14) | (t >> 21)) & 0xfu;
}

// the kept bytes of the word v at input index pos, bits 0-15: the rule, then
// nothing at or past n, and base 0 always
KMAN_DEV uint32_t keep16(const uint4 &v, uint32_t prev, uint64_t pos, uint64_t n) {
    uint32_t m = keep4(v.x, prev) | (keep4(v.y, v.x >> 24) << 4) | (keep4(v.z, v.y >> 24) << 8) |
                 (keep4(v.w, v.z >> 24) << 12);
    if (pos == 0) m |= 1u;
    const uint64_t left = pos < n ? n - pos : 0;
    if (left < 16) m &= (1u << (uint32_t)left) - 1u;
    return m;
}

template <bool MAP>
__global__ __launch_bounds__(HT) void hpc_compact_kernel(const uint8_t *__restrict__ codes, uint64_t n,
                                                         uint8_t *__restrict__ out, uint64_t *__restrict__ orig,
                                                         uint64_t *__restrict__ grp, uint64_t *status,
                                                         uint32_t *counter, uint32_t epoch, uint32_t *err) {
    __shared__ __attribute__((aligned(16))) uint8_t s_out[HTILE + 16];
    __shared__ uint16_t s_src[MAP ? HTILE : 1];
    __shared__ uint32_t lds_w[HT / 64];
    __shared__ uint64_t lds_base;
    __shared__ uint32_t lds_tile;
    const int64_t tile = grab_tile(counter, &lds_tile);
    const int lane = lane_id();
    const int w = threadIdx.x >> 6;
    const uint64_t wb = (uint64_t)tile * HTILE + (uint64_t)w * HWAVE;
    uint4 v[HG];
#pragma unroll
    for (int j = 0; j < HG; j++) v[j] = load16(codes, n, wb + (uint64_t)(j * 64 + lane) * 16);
    // the byte before the wave's first (wave-uniform; below n whenever the wave holds a base)
    uint32_t before = wb > 0 && wb - 1 < n ? codes[wb - 1] : 0u;
    uint32_t f[HG];
    uint64_t packed = 0;  // the kept bytes of word j in bits [16 j, 16 j + 16): a wave's sum is <= 1024 each
#pragma unroll
    for (int j = 0; j < HG; j++) {
        const uint32_t last = v[j].w >> 24;
        const uint32_t prev = wave_shr1(last, before);  // (lane 0 reads the fill)
        f[j] = keep16(v[j], prev, wb + (uint64_t)(j * 64 + lane) * 16, n);
        packed |= (uint64_t)__popc(f[j]) << (16 * j);
        before = (uint32_t)__builtin_amdgcn_readlane((int)last, 63);
    }
    const uint64_t inc = wave_inclusive_scan(packed, SumU64(), (uint64_t)0);
    const uint64_t tot = ((uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)(inc >> 32), 63) << 32) |
                         (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)inc, 63);
    const uint64_t exc = inc - packed;
    uint32_t wave_cnt = 0, goff[HG];  // goff[j]: the wave's kept bytes before this lane's word j
#pragma unroll
    for (int j = 0; j < HG; j++) {
        goff[j] = wave_cnt + (uint32_t)((exc >> (16 * j)) & 0xffffu);
        wave_cnt += (uint32_t)((tot >> (16 * j)) & 0xffffu);
    }
    if (lane == 0) lds_w[w] = wave_cnt;
    __syncthreads();
    uint32_t wpre = 0, tile_cnt = 0;
#pragma unroll
    for (int i = 0; i < HT / 64; i++) {
        const uint32_t x = lds_w[i];
        if (i < w) wpre += x;
        tile_cnt += x;
    }
    if (w == 0) {
        const uint64_t b = wave_lookback<0>(status, tile, tile_cnt, epoch, err);
        if (lane == 0) lds_base = b;
    }
    __syncthreads();
    const uint64_t base = lds_base;
    const uint32_t sh = (uint32_t)(base & 15u);
    // the kept bytes to (sh + tile-local rank) in LDS; the group prefixes
#pragma unroll
    for (int j = 0; j < HG; j++) {
        const uint32_t local = (uint32_t)w * HWAVE + (uint32_t)(j * 64 + lane) * 16;
        const uint64_t pos = (uint64_t)tile * HTILE + local;
        uint32_t o = wpre + goff[j];
        if ((lane & 15) == 0 && pos < n) grp[pos / GROUP] = base + o;
        const uint32_t x[4] = {v[j].x, v[j].y, v[j].z, v[j].w};
#pragma unroll
        for (int b = 0; b < 16; b++) {
            if ((f[j] >> b) & 1u) {
                s_out[sh + o] = (uint8_t)(x[b >> 2] >> (8 * (b & 3)));
                if constexpr (MAP) s_src[o] = (uint16_t)(local + b);
                o++;
            }
        }
    }
    __syncthreads();
    // out: the aligned words that hold [base, base + tile_cnt)
    const uint32_t span = sh + tile_cnt;
    uint8_t *__restrict__ dst = out + (base - sh);
    for (uint32_t lo = 16u * threadIdx.x; lo < span; lo += 16u * HT) {
        if (lo >= sh && lo + 16 <= span) {
            *reinterpret_cast<uint4 *>(dst + lo) = *reinterpret_cast<const uint4 *>(s_out + lo);
        } else {
#pragma unroll
            for (uint32_t b = 0; b < 16; b++)
                if (lo + b >= sh && lo + b < span) dst[lo + b] = s_out[lo + b];
        }
    }
    if constexpr (MAP) {
        const uint64_t t0 = (uint64_t)tile * HTILE;
        for (uint32_t q = threadIdx.x; q < tile_cnt; q += HT) orig[base + q] = t0 + s_src[q];
    }
}

// d_out_rec_seq[r]: the kept bases before min(rec_seq[r], n)
__global__ __launch_bounds__(HT) void hpc_table_kernel(const uint8_t *__restrict__ codes, uint64_t n,
                                                       const uint64_t *__restrict__ rec_seq, uint64_t n_records,
                                                       const uint64_t *__restrict__ grp, uint64_t total,
                                                       uint64_t *__restrict__ out_rec_seq) {
    const uint64_t r = (uint64_t)blockIdx.x * HT + threadIdx.x;
    if (r >= n_records) return;
    const uint64_t p = rec_seq[r];
    if (p >= n) {
        out_rec_seq[r] = total;
        return;
    }
    const uint64_t g0 = p & ~(uint64_t)(GROUP - 1);
    uint64_t acc = grp[g0 / GROUP];
    uint32_t prev = g0 > 0 ? codes[g0 - 1] : 0u;
    for (int s = 0; s < GROUP / 16; s++) {
        const uint64_t pos = g0 + 16ull * s;
        if (pos >= p) break;
        const uint4 v = load16(codes, n, pos);
        uint32_t m = keep16(v, prev, pos, n);
        if (p - pos < 16) m &= (1u << (uint32_t)(p - pos)) - 1u;
        acc += (uint32_t)__popc(m);
        prev = v.w >> 24;
    }
    out_rec_seq[r] = acc;
}

bool overlap(const void *a, uint64_t an, const void *b, uint64_t bn) {
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return x < y + bn && y < x + an;
}

}  // namespace

extern "C" int kman_hpc_records(kman_ctx *ctx, const uint8_t *d_codes, uint64_t n_bases, const uint64_t *d_rec_seq,
                                uint64_t n_records, uint8_t *d_out_codes, uint64_t *d_out_rec_seq, uint64_t *d_orig,
                                uint64_t *n_out) {
    if (!ctx || !n_out) return KMAN_EINVAL;
    *n_out = 0;
    if (!d_out_codes) return kman_fail(ctx, KMAN_EINVAL, "kman_hpc_records: null d_out_codes");
    if (n_bases && !d_codes) return kman_fail(ctx, KMAN_EINVAL, "kman_hpc_records: null d_codes");
    if (n_records && (!d_rec_seq || !d_out_rec_seq))
        return kman_fail(ctx, KMAN_EINVAL, "kman_hpc_records: null record table");
    if (((uintptr_t)d_codes & 15) != 0 || ((uintptr_t)d_out_codes & 15) != 0)
        return kman_fail(ctx, KMAN_EINVAL, "d_codes and d_out_codes must be 16-byte aligned");
    if (((uintptr_t)d_rec_seq & 7) != 0 || ((uintptr_t)d_out_rec_seq & 7) != 0 || ((uintptr_t)d_orig & 7) != 0)
        return kman_fail(ctx, KMAN_EINVAL, "d_rec_seq, d_out_rec_seq and d_orig must be 8-byte aligned");
    if (n_bases > (1ull << 56)) return kman_fail(ctx, KMAN_EINVAL, "kman_hpc_records: n_bases out of range");
    if (d_out_codes == d_codes || (n_bases && overlap(d_out_codes, n_bases + 64, d_codes, n_bases)))
        return kman_fail(ctx, KMAN_EINVAL, "kman_hpc_records does not run in place: d_out_codes lies over d_codes");
    const uint64_t T = ceil_div(n_bases, (uint64_t)HTILE), RB = ceil_div(n_records, (uint64_t)HT);
    if (T > 0x7fffffffull || RB > 0x7fffffffull)
        return kman_fail(ctx, KMAN_EINVAL, "%llu bases, %llu records: too many for one call",
                         (unsigned long long)n_bases, (unsigned long long)n_records);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    uint64_t total = 0;
    if (n_bases) {
        void *d_grp = nullptr;
        KMAN_TRY(kman_scratch(ctx, 8 * (size_t)ceil_div(n_bases, (uint64_t)GROUP), &d_grp));
        uint32_t epoch, *counter;
        KMAN_TRY(kman_lookback_begin(ctx, T, &epoch, &counter));
        {
            KTimer kt_(ctx, "hpc");
            if (d_orig)
                hipLaunchKernelGGL(hpc_compact_kernel<true>, dim3((uint32_t)T), dim3(HT), 0, ctx->stream, d_codes,
                                   n_bases, d_out_codes, d_orig, (uint64_t *)d_grp, ctx->d_status, counter, epoch,
                                   ctx->d_err);
            else
                hipLaunchKernelGGL(hpc_compact_kernel<false>, dim3((uint32_t)T), dim3(HT), 0, ctx->stream, d_codes,
                                   n_bases, d_out_codes, d_orig, (uint64_t *)d_grp, ctx->d_status, counter, epoch,
                                   ctx->d_err);
            HIP_TRY(ctx, hipGetLastError());
        }
        KMAN_TRY(kman_lookback_total(ctx, T, &total));  // (synchronises)
        if (n_records) {
            KTimer kt_(ctx, "hpc");
            hipLaunchKernelGGL(hpc_table_kernel, dim3((uint32_t)RB), dim3(HT), 0, ctx->stream, d_codes, n_bases,
                               d_rec_seq, n_records, (const uint64_t *)d_grp, total, d_out_rec_seq);
            HIP_TRY(ctx, hipGetLastError());
        }
    } else if (n_records) {
        HIP_TRY(ctx, hipMemsetAsync(d_out_rec_seq, 0, 8 * n_records, ctx->stream));
    }
    HIP_TRY(ctx, hipMemsetAsync(d_out_codes + total, 4, 64, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    *n_out = total;
    return KMAN_OK;
}
