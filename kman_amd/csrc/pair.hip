// pair.hip — the codes of two parsed inputs interleaved by record, R1[0] R2[0]
// R1[1] R2[1] .., in one buffer with one record table (`kmer screen --mate`,
// `kmer classify --mate`): a record-granular gather from two sources with any
// source and destination alignment.  Every second entry of the new table gives
// the lookup kernels pairs, every entry gives them mates.
//
// SEGMENT j of the output is mate 1 (j even) or mate 2 (j odd) of pair j / 2.
// A record table is already the exclusive scan of its records' lengths, so the
// output offsets are sums of entries of the two tables and nothing is scanned:
//
//   offsets  one thread per pair i, with a = min(d_rec_seq1[i], n_bases1),
//            b = min(d_rec_seq1[i + 1], n_bases1) (n_bases1 for the last pair)
//            and c = min(d_rec_seq2[i], n_bases2):
//            d_rec_seq[2i] = a + c, d_rec_seq[2i + 1] = b + c.  The end of the
//            last segment is n_bases1 + n_bases2.
//   copy     one block per KMAN_ZIP_TILE output bytes.  The block cuts the
//            slice of d_rec_seq that covers the tile with two block-wide upper
//            bounds (tile_records.h: 256 probes per step, at most 8 steps); a
//            slice of <= KMAN_ZIP_SEG_CAP segments is staged in LDS with the segments'
//            source offsets, a larger one (1-base and empty mates) is searched
//            in global memory.  A thread owns aligned 16-byte output words,
//            4096 B apart: an upper bound finds the word's segment, and the
//            word is put together PIECE by piece, a piece being the bytes of
//            one segment in the word: two aligned 16-byte loads of that
//            segment's source (one when source and destination agree mod 16),
//            a dword select, four v_alignbyte and a byte mask.  A word inside
//            one mate is one piece; a word of 1-base mates has sixteen.  One
//            16-byte store per word; the bytes of the last word at or past
//            the total are written as 4, the pad's value.
//   pad      the bytes from the last word's end to total + 64: a memset of 4.
//
// Bounds, not values: tile_records.h for the slice; table entries are clamped
// to n_bases; a source byte is read only below its n_bases (a byte that a wrong table asks for past it
// reads as 0); an output word is written only below total rounded up to 16,
// which the caller's total + 64 bytes hold.  Every search and every piece loop
// runs a step count fixed before it starts.
#include "bytes16.h"
#include "common.h"
#include "tile_records.h"

namespace {

constexpr int ZT = 256;
constexpr uint32_t TILE = KMAN_ZIP_TILE;
constexpr int SEG_CAP = KMAN_ZIP_SEG_CAP;
constexpr uint32_t PAD4 = 0x04040404u;
static_assert(TILE % (16 * ZT) == 0, "a tile is whole rounds of one 16-byte word per thread");

// the bytes [j0, j1) of a 16-byte word (0 <= j0 < j1 <= 16) that lie in its dword d, as a mask
KMAN_DEV uint32_t dword_mask(int j0, int j1, int d) {
    const int a = j0 - 4 * d > 0 ? j0 - 4 * d : 0;
    const int b = j1 - 4 * d < 4 ? j1 - 4 * d : 4;
    if (b <= a) return 0u;
    const uint32_t upto = b == 4 ? 0xffffffffu : (1u << (8 * b)) - 1u;
    return upto & ~((1u << (8 * a)) - 1u);  // (a <= 3)
}

__global__ __launch_bounds__(ZT) void zip_offsets_kernel(const uint64_t *__restrict__ rs1,
                                                         const uint64_t *__restrict__ rs2, uint64_t R, uint64_t n1,
                                                         uint64_t n2, uint64_t *__restrict__ out) {
    const uint64_t i = (uint64_t)blockIdx.x * ZT + threadIdx.x;
    if (i >= R) return;
    const uint64_t a = umin64(rs1[i], n1), b = i + 1 < R ? umin64(rs1[i + 1], n1) : n1, c = umin64(rs2[i], n2);
    out[2 * i] = a + c;
    out[2 * i + 1] = b + c;
}

// the output offset of segment j (j <= nseg; the end of the last one is the total) and its source offset
KMAN_DEV uint64_t seg_off(const uint64_t *__restrict__ O, uint64_t nseg, uint64_t total, uint64_t j) {
    const uint64_t v = O[j < nseg ? j : nseg - 1];  // (nseg >= 2)
    return j < nseg ? v : total;
}
KMAN_DEV uint64_t seg_src(const uint64_t *__restrict__ rs1, uint64_t n1, const uint64_t *__restrict__ rs2, uint64_t n2,
                          uint64_t j) {
    return (j & 1) ? umin64(rs2[j >> 1], n2) : umin64(rs1[j >> 1], n1);
}

// the tile's words.  Entry k of the slice is segment i0 + k: its offsets (ns + 1)
// and sources (ns) are sE and sS in LDS, or, BIG, read from the tables.
template <bool BIG>
KMAN_DEV void zip_words(const uint8_t *__restrict__ codes1, uint64_t n1, const uint8_t *__restrict__ codes2,
                        uint64_t n2, const uint64_t *__restrict__ rs1, const uint64_t *__restrict__ rs2,
                        const uint64_t *__restrict__ O, uint64_t nseg, uint64_t total, const uint64_t *sE,
                        const uint64_t *sS, uint64_t i0, uint64_t ns, uint64_t lo, uint64_t hi,
                        uint8_t *__restrict__ out) {
    auto off = [&](uint64_t k) -> uint64_t { return BIG ? seg_off(O, nseg, total, i0 + k) : sE[k]; };  // k <= ns
    auto source = [&](uint64_t k) -> uint64_t { return BIG ? seg_src(rs1, n1, rs2, n2, i0 + k) : sS[k]; };  // k < ns
    const uint64_t *es = BIG ? O + i0 : sE;  // (upper_count reads entries [0, ns) only, and i0 + ns <= nseg)
    for (uint64_t o = lo + 16ull * threadIdx.x; o < hi; o += 16ull * ZT) {
        const uint64_t wend = umin64(o + 16, hi);
        uint32_t x0 = PAD4, x1 = PAD4, x2 = PAD4, x3 = PAD4;  // (what no segment covers stays 4)
        uint64_t pos = o, cand = 0;  // cand - 1: the segment that starts at pos (0: not known)
        for (int it = 0; it < 17 && pos < wend; it++) {
            // the segment that holds pos: the one that starts there, or, when that one is empty, a search
            const uint64_t u = cand && cand <= ns && off(cand) > pos ? cand : upper_count(es, ns, pos);
            if (u == 0) {  // before the first segment (ns == 0: before the first entry, or the total)
                pos = umin64(off(0), wend);
                cand = 1;
                continue;
            }
            const uint64_t i = u - 1;
            cand = u + 1;
            const uint64_t seg = off(i), pe = umin64(off(i + 1), wend);
            if (pe <= pos) break;  // (a table that is not ascending)
            const bool second = ((i0 + i) & 1) != 0;
            const uint8_t *__restrict__ src = second ? codes2 : codes1;
            const uint64_t n = second ? n2 : n1;
            const uint64_t sa = source(i) + (pos - seg);  // the source index of output byte pos
            const int j0 = (int)(pos - o), j1 = (int)(pe - o);
            uint4 v;
            if (sa >= (uint64_t)j0) {
                v = shifted16(src, n, sa - (uint64_t)j0);
            } else {  // (the first bytes of a source: the shifted word would start before it)
                auto dword = [&](int d) -> uint32_t {
                    uint32_t acc = 0;
#pragma unroll
                    for (int b = 0; b < 4; b++) {
                        const int j = 4 * d + b;
                        const uint64_t q = sa + (uint64_t)(j - j0);
                        if (j >= j0 && j < j1 && q < n) acc |= (uint32_t)src[q] << (8 * b);
                    }
                    return acc;
                };
                v = make_uint4(dword(0), dword(1), dword(2), dword(3));
            }
            const uint32_t m0 = dword_mask(j0, j1, 0), m1 = dword_mask(j0, j1, 1), m2 = dword_mask(j0, j1, 2),
                           m3 = dword_mask(j0, j1, 3);
            x0 = (x0 & ~m0) | (v.x & m0);
            x1 = (x1 & ~m1) | (v.y & m1);
            x2 = (x2 & ~m2) | (v.z & m2);
            x3 = (x3 & ~m3) | (v.w & m3);
            pos = pe;
        }
        *reinterpret_cast<uint4 *>(out + o) = make_uint4(x0, x1, x2, x3);
    }
}

__global__ __launch_bounds__(ZT) void zip_copy_kernel(const uint8_t *__restrict__ codes1, uint64_t n1,
                                                      const uint8_t *__restrict__ codes2, uint64_t n2,
                                                      const uint64_t *__restrict__ rs1,
                                                      const uint64_t *__restrict__ rs2,
                                                      const uint64_t *__restrict__ O, uint64_t nseg, uint64_t total,
                                                      uint8_t *__restrict__ out) {
    __shared__ uint64_t sE[SEG_CAP + 1];
    __shared__ uint64_t sS[SEG_CAP];
    __shared__ uint32_t s_cnt[ZT / 64];
    const uint64_t lo = (uint64_t)blockIdx.x * TILE;
    const uint64_t hi = umin64(lo + TILE, total);  // (lo < total: the grid is ceil(total / TILE))
    // the segments that hold output bytes [lo, hi): from the last one that
    // starts at or before lo to the last one that starts at or before hi - 1
    const uint64_t u0 = block_upper_count<ZT>(O, nseg, lo, s_cnt), u1 = block_upper_count<ZT>(O, nseg, hi - 1, s_cnt);
    const TileSlice sl = slice_of(u0, u1);
    const uint64_t i0 = sl.r0, ns = sl.ns;  // (ns == 0: the tile lies before the first segment)
    if (ns > (uint64_t)SEG_CAP) {
        zip_words<true>(codes1, n1, codes2, n2, rs1, rs2, O, nseg, total, nullptr, nullptr, i0, ns, lo, hi, out);
        return;
    }
    for (uint32_t i = threadIdx.x; i <= (uint32_t)ns; i += ZT) sE[i] = seg_off(O, nseg, total, i0 + i);
    for (uint32_t i = threadIdx.x; i < (uint32_t)ns; i += ZT) sS[i] = seg_src(rs1, n1, rs2, n2, i0 + i);
    __syncthreads();
    zip_words<false>(codes1, n1, codes2, n2, rs1, rs2, O, nseg, total, sE, sS, i0, ns, lo, hi, out);
}

}  // namespace

extern "C" int kman_zip_records(kman_ctx *ctx, const uint8_t *d_codes1, uint64_t n_bases1, const uint64_t *d_rec_seq1,
                                const uint8_t *d_codes2, uint64_t n_bases2, const uint64_t *d_rec_seq2,
                                uint64_t n_records, uint8_t *d_codes, uint64_t *d_rec_seq) {
    if (!ctx) return KMAN_EINVAL;
    if (!d_codes) return kman_fail(ctx, KMAN_EINVAL, "kman_zip_records: null d_codes");
    if (n_records && (!d_rec_seq1 || !d_rec_seq2 || !d_rec_seq))
        return kman_fail(ctx, KMAN_EINVAL, "kman_zip_records: null record table");
    if ((n_bases1 && !d_codes1) || (n_bases2 && !d_codes2))
        return kman_fail(ctx, KMAN_EINVAL, "kman_zip_records: null codes");
    if (((uintptr_t)d_codes1 & 15) != 0 || ((uintptr_t)d_codes2 & 15) != 0 || ((uintptr_t)d_codes & 15) != 0)
        return kman_fail(ctx, KMAN_EINVAL, "d_codes1, d_codes2 and d_codes must be 16-byte aligned");
    if (n_records > (1ull << 31))
        return kman_fail(ctx, KMAN_EINVAL, "%llu pairs: too many", (unsigned long long)n_records);
    if (n_bases1 > (1ull << 62) || n_bases2 > (1ull << 62))
        return kman_fail(ctx, KMAN_EINVAL, "kman_zip_records: n_bases out of range");
    const uint64_t total = n_records ? n_bases1 + n_bases2 : 0;  // (no pairs: no record owns a base)
    const uint64_t blocks = ceil_div(total, (uint64_t)TILE);
    if (blocks > 0x7fffffffull)
        return kman_fail(ctx, KMAN_EINVAL, "%llu bases: too many for one call", (unsigned long long)total);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const uint64_t body = (total + 15) & ~15ull;  // the copy pass writes whole words
    if (total) {
        KTimer kt_(ctx, "zip");
        hipLaunchKernelGGL(zip_offsets_kernel, dim3((uint32_t)ceil_div(n_records, (uint64_t)ZT)), dim3(ZT), 0,
                           ctx->stream, d_rec_seq1, d_rec_seq2, n_records, n_bases1, n_bases2, d_rec_seq);
        HIP_TRY(ctx, hipGetLastError());
        hipLaunchKernelGGL(zip_copy_kernel, dim3((uint32_t)blocks), dim3(ZT), 0, ctx->stream, d_codes1, n_bases1,
                           d_codes2, n_bases2, d_rec_seq1, d_rec_seq2, d_rec_seq, 2 * n_records, total, d_codes);
        HIP_TRY(ctx, hipGetLastError());
    } else if (n_records) {  // (every mate is empty: the table is all zeros)
        HIP_TRY(ctx, hipMemsetAsync(d_rec_seq, 0, 16 * n_records, ctx->stream));
    }
    HIP_TRY(ctx, hipMemsetAsync(d_codes + body, 4, total + 64 - body, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return KMAN_OK;
}
