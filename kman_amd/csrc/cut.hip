// cut.hip — the listed records of the input text, whole or cut to one column
// interval, written as one contiguous text on the device (`kmer screen
// --reads-out`, `--trim`): a stream compaction of byte ranges of any length
// with any source and destination alignment.
//
// The text is described as SEGMENTS (src, out_len): out_len output bytes that
// are out_len text bytes from src on (whole records, one segment per record)
// or, under KMAN_CUT_TRIM, out_len - 1 text bytes and one "\n" (four segments
// per record: line 1, line 2 cut, line 3, line 4 cut).  A record that is not
// written has out_len 0 in every segment.  Work memory: E, nseg + 1 u64
// (out_len, then its exclusive scan, E[nseg] the text size) and src, nseg u64.
//
//   whole   (pass 1) one thread per record: the clamped range.
//   trim    (pass 1) one wave per record, 64 lanes x 16 B = 1024 text bytes per
//           step, every load a 16-byte word of the text.  Walk 1 stops at the
//           record's fourth line end: a lane marks the bytes that start a
//           terminator ("\r", or "\n" not after "\r"), a ballot finds the lanes
//           that have one.  Walk 2 covers line 2 once: the lane's not-blank
//           bytes are counted (popcount, a DPP wave scan, a running total), the
//           lanes that hold the START-th and the (END - 1)-th of them note
//           their position, every lane notes its last byte that the right
//           strip keeps; three wave reductions after the walk.  A record of L
//           bytes takes about L / 1024 steps of one wave whatever its length;
//           there is no block-per-record path for very long reads.
//   scan    E in place, tiles of 2048 entries, the decoupled look-back of
//           common.h (the format kernels' scan); its last status word is the
//           text size.
//   copy    (pass 2) one block per KMAN_CUT_TILE output bytes.  Thread 0 cuts
//           the slice of E that covers the tile (tile_records.h); a slice of
//           <= KMAN_CUT_SEG_CAP segments is staged in LDS, a larger one (many
//           records of a few bytes, or long rows of unlisted ones) is searched
//           in global memory.  A thread owns 16-byte output words, 4096 B
//           apart: an upper bound finds the word's segment.  A word inside one
//           segment's text bytes is two 16-byte text loads (one when the source
//           is aligned too), a dword select and four v_alignbyte, one 16-byte
//           store.  A word that holds a segment's end or its "\n" is put
//           together byte by byte (the next segment first, a search when that
//           one is empty) and still stored as one word; byte stores happen only
//           in the text's last word.  Work per block does not depend on the
//           records' lengths.
//
// Bounds, not values: tile_records.h for the slice of E; record offsets are
// clamped to n_bytes and a descending pair is an empty record; every line search ends at the record's end; a text
// byte is read only below n_bytes, an output byte written only below the text
// size, which the host has checked against cap before pass 2 is launched.
#include "bytes16.h"
#include "common.h"
#include "tile_records.h"

namespace {

constexpr int CT = 256;
constexpr uint32_t TILE = KMAN_CUT_TILE;
constexpr int SEG_CAP = KMAN_CUT_SEG_CAP;
constexpr int SCAN_E = 8;
constexpr int SCAN_TILE = CT * SCAN_E;
constexpr uint64_t NOPOS = ~0ull;
static_assert(TILE % (16 * CT) == 0, "a tile is whole rounds of one 16-byte word per thread");

// what the parser's right strip removes from a sequence line
KMAN_DEV bool is_strip(uint32_t c) { return c == ' ' || c == '\t' || c == 0x0b || c == 0x0c || (c >= 0x1c && c <= 0x1f); }

// the position of the n-th (from 0) set bit of m; n < popcount(m)
KMAN_DEV uint32_t nth_bit(uint32_t m, uint32_t n) {
#pragma unroll
    for (int j = 0; j < 16; j++) {
        if (j >= (int)n) break;
        m &= m - 1;
    }
    return (uint32_t)__ffs((int)m) - 1u;
}

KMAN_DEV uint64_t wave_max(uint64_t v) { return wave_reduce_lb<1>(v); }
KMAN_DEV uint64_t wave_min(uint64_t v) { return ~wave_reduce_lb<1>(~v); }

// pass 1, whole records
__global__ __launch_bounds__(CT) void cut_whole_kernel(const uint64_t *__restrict__ rec_off, uint64_t n_records,
                                                       const uint8_t *__restrict__ keep, uint64_t n_bytes,
                                                       uint64_t *__restrict__ E, uint64_t *__restrict__ src) {
    const uint64_t r = (uint64_t)blockIdx.x * CT + threadIdx.x;
    if (r >= n_records) return;
    const uint64_t a = umin64(rec_off[r], n_bytes), b = umin64(rec_off[r + 1], n_bytes);
    const bool kept = !keep || keep[r] != 0;
    E[r] = kept && b > a ? b - a : 0;
    src[r] = a;
}

// pass 1, trimmed FASTQ records: one wave per record
__global__ __launch_bounds__(CT) void cut_trim_kernel(const uint8_t *__restrict__ text, uint64_t n_bytes,
                                                      const uint64_t *__restrict__ rec_off, uint64_t n_records,
                                                      const uint8_t *__restrict__ keep,
                                                      const uint64_t *__restrict__ start,
                                                      const uint64_t *__restrict__ end, uint64_t *__restrict__ E,
                                                      uint64_t *__restrict__ src) {
    const uint64_t r = (uint64_t)blockIdx.x * (CT / 64) + (threadIdx.x >> 6);
    if (r >= n_records) return;  // (the whole wave)
    const int lane = lane_id();
    const uint64_t a = umin64(rec_off[r], n_bytes), b = umin64(rec_off[r + 1], n_bytes);
    const uint64_t S = start[r], En = end[r];
    const bool live = (!keep || keep[r] != 0) && b > a && S < En;
    uint64_t so[4] = {a, a, a, a}, ol[4] = {0, 0, 0, 0};
    if (live) {
        // walk 1: the record's first four terminator starts (b: the line runs to the record's end)
        uint64_t t0 = b, t1 = b, t2 = b, t3 = b;
        uint32_t found = 0;
        for (uint64_t base = a & ~15ull; base < b && found < 4; base += 1024) {
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
            while (bal && found < 4) {
                const int L = __ffsll((unsigned long long)bal) - 1;
                uint32_t lm = (uint32_t)__shfl((int)m, L, 64);
                while (lm && found < 4) {
                    const uint64_t pos = base + 16ull * (uint32_t)L + ((uint32_t)__ffs((int)lm) - 1u);
                    if (found == 0) t0 = pos;
                    else if (found == 1) t1 = pos;
                    else if (found == 2) t2 = pos;
                    else t3 = pos;
                    found++;
                    lm &= lm - 1;
                }
                bal &= bal - 1;
            }
        }
        const uint64_t s2 = line_after(text, t0, b), s3 = line_after(text, t1, b), s4 = line_after(text, t2, b);
        const uint64_t e2 = t1;
        // walk 2 over line 2
        uint64_t pS = NOPOS, pE = NOPOS, last = 0, seen = 0;
        for (uint64_t base = s2 & ~15ull; base < e2; base += 1024) {
            const uint64_t p = base + 16ull * (uint32_t)lane;
            uint32_t nb = 0, ns = 0;
            if (p < e2) {
                const uint4 v = load16(text, n_bytes, p);
#pragma unroll
                for (int j = 0; j < 16; j++) {
                    const uint32_t c = byte_of(v, j);
                    const uint64_t pos = p + j;
                    if (pos >= s2 && pos < e2) {
                        if (c != ' ') nb |= 1u << j;
                        if (!is_strip(c)) ns |= 1u << j;
                    }
                }
            }
            const uint32_t cnt = (uint32_t)__popc(nb);
            const uint32_t inc = wave_inclusive_scan(cnt, SumU32(), 0u);
            const uint64_t pre = seen + (inc - cnt);
            if (S >= pre && S - pre < cnt) pS = p + nth_bit(nb, (uint32_t)(S - pre));
            if (En - 1 >= pre && En - 1 - pre < cnt) pE = p + nth_bit(nb, (uint32_t)(En - 1 - pre));
            if (ns) last = p + (32u - (uint32_t)__clz((int)ns));
            seen += (uint32_t)__shfl((int)inc, 63, 64);
        }
        pS = wave_min(pS);
        pE = wave_min(pE);
        const uint64_t body_end = wave_max(last);  // (0: nothing is left of line 2)
        if (pS != NOPOS && pS < body_end) {        // START < len(cols)
            const uint64_t c0 = pS, c1 = pE != NOPOS && pE < body_end ? pE + 1 : body_end;  // END clamped
            const uint64_t len4 = t3 - s4;
            const uint64_t q0 = umin64(c0 - s2, len4), q1 = umin64(c1 - s2, len4);
            so[0] = a, ol[0] = t0 - a + 1;
            so[1] = c0, ol[1] = c1 - c0 + 1;
            so[2] = s3, ol[2] = t2 - s3 + 1;
            so[3] = s4 + q0, ol[3] = q1 - q0 + 1;
        }
    }
    if (lane < 4) {
        const uint64_t s = lane == 0 ? so[0] : lane == 1 ? so[1] : lane == 2 ? so[2] : so[3];
        const uint64_t l = lane == 0 ? ol[0] : lane == 1 ? ol[1] : lane == 2 ? ol[2] : ol[3];
        E[4 * r + lane] = l;
        src[4 * r + lane] = s;
    }
}

// E[0, n] <- the exclusive sums of E[0, n) (E[n]: the total), in place
__global__ __launch_bounds__(CT) void cut_scan_kernel(uint64_t *__restrict__ E, uint64_t n,
                                                      uint64_t *__restrict__ status, uint32_t *__restrict__ counter,
                                                      uint32_t epoch, uint32_t *__restrict__ err) {
    __shared__ uint64_t lds_scan[CT / 64];
    __shared__ uint64_t lds_base;
    __shared__ uint32_t lds_tile;
    const int64_t tile = grab_tile(counter, &lds_tile);
    const uint64_t i0 = (uint64_t)tile * SCAN_TILE + (uint64_t)threadIdx.x * SCAN_E;
    uint64_t v[SCAN_E], mine = 0;
#pragma unroll
    for (int q = 0; q < SCAN_E; q++) {
        v[q] = i0 + q < n ? E[i0 + q] : 0;
        mine += v[q];
    }
    uint64_t total;
    const uint64_t ex = block_exclusive_scan<CT>(mine, SumU64(), (uint64_t)0, lds_scan, &total);
    if (threadIdx.x < 64) {
        const uint64_t b = wave_lookback<0>(status, tile, total, epoch, err);
        if (threadIdx.x == 0) lds_base = b;
    }
    __syncthreads();
    uint64_t run = lds_base + ex;
#pragma unroll
    for (int q = 0; q < SCAN_E; q++) {
        if (i0 + q <= n) E[i0 + q] = run;
        run += v[q];
    }
}

// pass 2
__global__ __launch_bounds__(CT) void cut_copy_kernel(const uint8_t *__restrict__ text, uint64_t n_bytes,
                                                      const uint64_t *__restrict__ E, const uint64_t *__restrict__ src,
                                                      uint64_t nseg, uint64_t total, uint32_t nl,
                                                      uint8_t *__restrict__ out) {
    __shared__ uint64_t sE[SEG_CAP + 1];
    __shared__ uint64_t sS[SEG_CAP];
    __shared__ uint64_t s_i0, s_ns;
    const uint64_t lo = (uint64_t)blockIdx.x * TILE;
    const uint64_t hi = umin64(lo + TILE, total);  // (lo < total: the grid is ceil(total / TILE))
    if (threadIdx.x == 0) {
        const TileSlice s = cut_slice(E, nseg, lo, hi - 1);  // the segments that hold output bytes [lo, hi)
        s_i0 = s.r0;
        s_ns = s.ns;
    }
    __syncthreads();
    const uint64_t i0 = s_i0, ns = s_ns;
    if (ns == 0) return;  // (cannot happen: E[0] = 0 <= lo)
    // (E has nseg + 1 entries and i0 + ns <= nseg: the tail is E's own entry)
    const uint64_t *es = stage_slice<CT, SEG_CAP, TAIL_ENTRY>(E, {i0, ns, 0}, sE).rs;
    const uint64_t *ss = stage_slice<CT, SEG_CAP>(src, {i0, ns, 0}, sS).rs;
    if (ns <= (uint64_t)SEG_CAP) __syncthreads();  // (block-uniform)

    for (uint64_t o = lo + 16ull * threadIdx.x; o < hi; o += 16ull * CT) {
        const uint64_t u = upper_count(es, ns, o);
        uint64_t i = u ? u - 1 : 0;
        uint64_t seg = es[i], end = es[i + 1];
        const uint64_t s = ss[i] + (o - seg);
        if (o + 16 <= hi && o >= seg && o + 16 + nl <= end && s + 16 <= n_bytes) {
            // sixteen text bytes of one segment
            *reinterpret_cast<uint4 *>(out + o) = shifted16(text, n_bytes, s);
            continue;
        }
        uint32_t x[4] = {0, 0, 0, 0};
#pragma unroll
        for (int j = 0; j < 16; j++) {
            const uint64_t pos = o + j;
            if (pos >= hi) continue;
            if (pos >= end) {
                // the next segment, or, when that one is empty, the one that holds pos
                uint64_t k = i + 1;
                if (!(k < ns && es[k + 1] > pos)) {
                    const uint64_t uu = upper_count(es, ns, pos);
                    k = uu ? uu - 1 : 0;
                }
                i = k;
                seg = es[i];
                end = es[i + 1];
            }
            uint32_t c = '\n';
            if (!(nl && pos + 1 == end)) {
                const uint64_t sa = ss[i] + (pos - seg);
                c = sa < n_bytes ? text[sa] : 0u;
            }
            x[j >> 2] |= c << (8 * (j & 3));
        }
        if (o + 16 <= hi) {
            *reinterpret_cast<uint4 *>(out + o) = make_uint4(x[0], x[1], x[2], x[3]);
        } else {
#pragma unroll
            for (int j = 0; j < 16; j++)
                if (o + j < hi) out[o + j] = (uint8_t)(x[j >> 2] >> (8 * (j & 3)));
        }
    }
}

uint64_t segs_of(uint64_t n_records, uint32_t flags) { return n_records * ((flags & KMAN_CUT_TRIM) ? 4u : 1u); }

}  // namespace

extern "C" int kman_cut_records_plan(uint64_t n_records, uint32_t flags, uint64_t *work_bytes) {
    if (!work_bytes) return KMAN_EINVAL;
    *work_bytes = 0;
    if ((flags & ~KMAN_CUT_TRIM) != 0 || n_records > (1ull << 31)) return KMAN_EINVAL;  // (the grids)
    const uint64_t b = 8 * (2 * segs_of(n_records, flags) + 1);
    *work_bytes = (b + 15) & ~15ull;
    return KMAN_OK;
}

extern "C" int kman_cut_records(kman_ctx *ctx, const uint8_t *d_text, uint64_t n_bytes, const uint64_t *d_rec_off,
                                uint64_t n_records, const uint8_t *d_keep, const uint64_t *d_start,
                                const uint64_t *d_end, uint32_t flags, void *d_work, uint64_t work_bytes, char *d_out,
                                size_t cap, size_t *used) {
    if (!ctx || !used) return KMAN_EINVAL;
    *used = 0;
    if ((flags & ~KMAN_CUT_TRIM) != 0) return kman_fail(ctx, KMAN_EINVAL, "kman_cut_records: unknown flags %u", flags);
    const bool trim = (flags & KMAN_CUT_TRIM) != 0;
    if (!trim && (d_start || d_end))
        return kman_fail(ctx, KMAN_EINVAL, "kman_cut_records: d_start / d_end without KMAN_CUT_TRIM");
    if (n_records == 0) return KMAN_OK;
    if (!d_rec_off || !d_work || (n_bytes && !d_text) || (trim && (!d_start || !d_end)))
        return kman_fail(ctx, KMAN_EINVAL, "kman_cut_records: null buffer");
    if (((uintptr_t)d_text & 15) != 0 || ((uintptr_t)d_out & 15) != 0 || ((uintptr_t)d_work & 15) != 0)
        return kman_fail(ctx, KMAN_EINVAL, "d_text, d_out and d_work must be 16-byte aligned");
    uint64_t want = 0;
    if (kman_cut_records_plan(n_records, flags, &want) != KMAN_OK)
        return kman_fail(ctx, KMAN_EINVAL, "%llu records: too many", (unsigned long long)n_records);
    if (work_bytes < want)
        return kman_fail(ctx, KMAN_ECAP, "work buffer of %llu bytes: kman_cut_records_plan asks for %llu",
                         (unsigned long long)work_bytes, (unsigned long long)want);
    if (n_bytes == 0) return KMAN_OK;  // (every record is empty)
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const uint64_t nseg = segs_of(n_records, flags);
    uint64_t *d_E = (uint64_t *)d_work, *d_src = d_E + nseg + 1;
    const uint64_t tiles = ceil_div(nseg + 1, (uint64_t)SCAN_TILE);
    uint32_t epoch, *counter;
    KMAN_TRY(kman_lookback_begin(ctx, tiles, &epoch, &counter));
    {
        KTimer kt_(ctx, "cut_records");
        if (trim)
            hipLaunchKernelGGL(cut_trim_kernel, dim3((uint32_t)ceil_div(n_records, CT / 64)), dim3(CT), 0, ctx->stream,
                               d_text, n_bytes, d_rec_off, n_records, d_keep, d_start, d_end, d_E, d_src);
        else
            hipLaunchKernelGGL(cut_whole_kernel, dim3((uint32_t)ceil_div(n_records, CT)), dim3(CT), 0, ctx->stream,
                               d_rec_off, n_records, d_keep, n_bytes, d_E, d_src);
        HIP_TRY(ctx, hipGetLastError());
        hipLaunchKernelGGL(cut_scan_kernel, dim3((uint32_t)tiles), dim3(CT), 0, ctx->stream, d_E, nseg, ctx->d_status,
                           counter, epoch, ctx->d_err);
        HIP_TRY(ctx, hipGetLastError());
    }
    uint64_t tot = 0;
    KMAN_TRY(kman_lookback_total(ctx, tiles, &tot));  // (synchronises)
    *used = (size_t)tot;
    if (tot > (d_out ? (uint64_t)cap : 0)) return KMAN_ECAP;  // (sizing, or too small: nothing is written)
    if (tot == 0) return KMAN_OK;
    const uint64_t blocks = ceil_div(tot, (uint64_t)TILE);
    if (blocks > 0x7fffffffull) return kman_fail(ctx, KMAN_EINVAL, "a text of %llu bytes: too long for one call",
                                                 (unsigned long long)tot);
    {
        KTimer kt_(ctx, "cut_records");
        hipLaunchKernelGGL(cut_copy_kernel, dim3((uint32_t)blocks), dim3(CT), 0, ctx->stream, d_text, n_bytes, d_E,
                           d_src, nseg, tot, trim ? 1u : 0u, reinterpret_cast<uint8_t *>(d_out));
        HIP_TRY(ctx, hipGetLastError());
    }
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return KMAN_OK;
}
