// screen_lookup.h — the table lookup that the kernels over a count table share
// (screen.hip, quantile.hip, classify.hip, correct.hip, unitig.hip): a thread's
// EI windows against a key-sorted table through the prefix index of
// kman_table_index.  table_rows is the search, table_lookup reads the count of
// the row it ends on.
//
// The EI searches advance in lockstep: the EI index pairs are loaded, then
// step 1 of all EI searches, then step 2, ..: EI independent loads in flight
// per thread, not EI dependent chains one after another.  A search halves its
// bucket; the step count is bits(largest bucket of the thread) <= 64.  A probe
// that reads the key itself marks the hit (a lower bound that ends inside the
// bucket has probed the row it ends on), so a bucket of n rows costs
// floor(log2 n) + 1 key reads, and a hit one count read.
//
// Bounds, not values: lo <= hi <= nt are clamped after loading, every key and
// count index is < nt; keys 0 and 2^64 - 1 are ordinary keys.  An index that
// does not belong to the table, or keys that are not ascending, give wrong
// counts but no wild address and no unbounded loop.
#pragma once
#include "common.h"

namespace {

// halvings that empty a range of len rows: bits(len), 0 for an empty one
KMAN_DEV uint32_t steps_of(uint64_t len) { return len ? 64u - (uint32_t)__builtin_clzll(len) : 0u; }

inline bool index_bits_ok(uint32_t k, uint32_t index_bits) {
    const uint32_t top = 2 * k < KMAN_SCREEN_MAX_INDEX_BITS ? 2 * k : KMAN_SCREEN_MAX_INDEX_BITS;
    return index_bits >= 1 && index_bits <= top;
}

// The lockstep search.  The windows j with bit j of `valid` set are looked up
// by kf[j]; returns the mask of those that are rows of the table, and row[j] =
// where window j's lower bound ended: row[j] < nt for every bit of the mask.
template <int EI>
KMAN_DEV uint32_t table_rows(uint32_t valid, const uint64_t (&kf)[EI], uint32_t shift,
                             const uint64_t *__restrict__ index, const uint64_t *__restrict__ tkeys, uint64_t nt,
                             uint64_t (&row)[EI]) {
    uint64_t (&lo)[EI] = row;
    uint64_t len[EI];
#pragma unroll
    for (int j = 0; j < EI; j++) {
        const bool ok = (valid >> j) & 1u;
        const uint64_t p = kf[j] >> shift;
        lo[j] = ok ? index[p] : 0;
        len[j] = ok ? index[p + 1] : 0;
    }
    uint32_t nsteps = 0;
#pragma unroll
    for (int j = 0; j < EI; j++) {
        const uint64_t hi = umin64(len[j], nt);  // lo <= hi <= nt whatever the index holds
        lo[j] = umin64(lo[j], hi);
        len[j] = hi - lo[j];
        const uint32_t s = steps_of(len[j]);
        nsteps = s > nsteps ? s : nsteps;
    }
    uint32_t hit = 0;
    for (uint32_t s = 0; s < nsteps; s++) {  // (nsteps <= 64)
        uint64_t v[EI];
#pragma unroll
        for (int j = 0; j < EI; j++) v[j] = len[j] ? tkeys[lo[j] + (len[j] >> 1)] : 0;  // (lo + half < lo + len <= nt)
#pragma unroll
        for (int j = 0; j < EI; j++) {
            const uint64_t half = len[j] >> 1;
            const bool on = len[j] != 0;
            hit |= (uint32_t)(on && v[j] == kf[j]) << j;
            if (on && v[j] < kf[j]) {
                lo[j] += half + 1;
                len[j] -= half + 1;
            } else {
                len[j] = half;
            }
        }
    }
    // a hit's row is where its lower bound ended (the search never passes the row it has probed: lo < nt then)
    uint32_t ok = 0;
#pragma unroll
    for (int j = 0; j < EI; j++) ok |= (uint32_t)(((hit >> j) & 1u) && lo[j] < nt) << j;
    return ok;
}

// table_rows with the hit row's count: cnt[j] = the row's count (0 for the others)
template <int EI, typename CT>
KMAN_DEV uint32_t table_lookup(uint32_t valid, const uint64_t (&kf)[EI], uint32_t shift,
                               const uint64_t *__restrict__ index, const uint64_t *__restrict__ tkeys,
                               const CT *__restrict__ tcounts, uint64_t nt, uint64_t (&cnt)[EI]) {
    uint64_t row[EI];
    const uint32_t hit = table_rows<EI>(valid, kf, shift, index, tkeys, nt, row);
#pragma unroll
    for (int j = 0; j < EI; j++) cnt[j] = (hit >> j) & 1u ? (uint64_t)tcounts[row[j]] : 0;
    return hit;
}

}  // namespace
