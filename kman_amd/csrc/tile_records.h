// tile_records.h — the sorted-boundary-table layer of the kernels that work on
// tiles of a stream cut into records or segments (screen.hip, classify.hip,
// runs.hip, correct.hip over d_rec_seq; cut.hip and pair.hip over their segment
// tables; quantile.hip for the counts alone).
//
// A table of n ascending u64 says where each record starts; record i owns the
// positions [table[i], table[i + 1]).  One block works on the positions
// [first, last] of its tile:
//   cut     thread 0 runs two upper bounds (cut_slice): the SLICE is entries
//           [r0, r0 + ns), from the owner of `first` (or entry 0, when nothing
//           starts at or before `first`) to the owner of `last`; ns == 0 when
//           nothing starts at or before `last`.  Where asked it also takes
//           `next`, the first position after the slice: entry r0 + ns clamped
//           to a limit, or the limit when the table ends there.
//   stage   a slice of <= CAP entries is copied to LDS (stage_slice), a larger
//           one (many empty or one-position records) stays in global memory;
//           either way the kernel goes on with rs[0, ns) and the flag `big`.
//           stage_slice has no barrier: the kernel publishes the LDS copy with
//           a barrier of its own.
//   walk    owner_walk: a thread's EI consecutive windows, added up per run of
//           one owner (screen.hip and classify.hip).
//
// Bounds, not values.  Nothing here trusts what the table holds, only how long
// it is:
//   - upper_count, lower_count and block_upper_count read entries [0, n) only
//     and run a step count fixed before they start (64 halvings, 8 rounds of
//     NT chunks), so every count is <= n whatever the order of the entries;
//   - r0 + ns <= n follows from u0, u1 <= n, so a slice index i < ns addresses
//     table[r0 + i] inside the table and record r0 + i < n; entry r0 + ns is
//     read only after r0 + ns < n has been checked (or, TAIL_ENTRY, from a
//     table that has n + 1 entries);
//   - stage_slice copies only when ns <= CAP (+ 1 with a tail) into an array
//     the caller has declared with that many entries;
//   - in owner_walk u <= ns, rs[u] is read only where u < ns, and a slot is
//     used only after slot < CAP has been tested; the global path's slot is
//     the owner's first position in the tile, taken as 0 when the entry lies
//     before the tile, so it is < the tile size only through that test.
// An unsorted table therefore gives wrong owners (wrong or unwritten results),
// never a wild address or an unbounded loop.  What a kernel does with an
// owner (output indices, positions clamped to n_bases) is checked in that
// kernel and stated at the top of its file.
#pragma once
#include "common.h"

namespace {

// the number of entries of rs[0, n) that are <= b
KMAN_DEV uint64_t upper_count(const uint64_t *rs, uint64_t n, uint64_t b) {
    uint64_t lo = 0, len = n;
    for (int s = 0; s < 64 && len; s++) {
        const uint64_t half = len >> 1;
        if (rs[lo + half] <= b) {
            lo += half + 1;
            len -= half + 1;
        } else {
            len = half;
        }
    }
    return lo;
}

// the number of entries of rs[0, n) that are < x
KMAN_DEV uint64_t lower_count(const uint64_t *rs, uint64_t n, uint64_t x) {
    uint64_t lo = 0, len = n;
    for (int s = 0; s < 64 && len; s++) {
        const uint64_t half = len >> 1;
        if (rs[lo + half] < x) {
            lo += half + 1;
            len -= half + 1;
        } else {
            len = half;
        }
    }
    return lo;
}

// upper_count by a whole block of NT threads: every step probes the last entry
// of NT equal chunks of the range and keeps the first chunk whose last entry
// is > b (8 steps cover 2^64 entries).  Every thread returns the same number.
// lds_cnt: NT / 64 words; two barriers per step.
template <int NT>
KMAN_DEV uint64_t block_upper_count(const uint64_t *__restrict__ e, uint64_t n, uint64_t b, uint32_t *lds_cnt) {
    uint64_t lo = 0, len = n;
    for (int s = 0; s < 8 && len; s++) {
        const uint64_t chunk = (len + NT - 1) / NT;
        const uint64_t first = (uint64_t)threadIdx.x * chunk;
        bool le = false;
        if (first < len) le = e[lo + umin64(first + chunk, len) - 1] <= b;
        const uint64_t bal = __ballot(le);
        if (lane_id() == 0) lds_cnt[threadIdx.x >> 6] = (uint32_t)__popcll((unsigned long long)bal);
        __syncthreads();
        uint32_t c = 0;
#pragma unroll
        for (int w = 0; w < NT / 64; w++) c += lds_cnt[w];
        __syncthreads();
        // chunks [0, c) are <= b throughout (ascending entries); the answer lies in chunk c, before its last entry
        const uint64_t skip = umin64((uint64_t)c * chunk, len);
        lo += skip;
        len -= skip;
        len = len ? umin64(chunk, len) - 1 : 0;
    }
    return lo;
}

// entries [r0, r0 + ns) of a table; next: the first position after them (0 where it was not asked for)
struct TileSlice {
    uint64_t r0, ns, next;
};

// from the two upper counts of a tile's first and last position
KMAN_DEV TileSlice slice_of(uint64_t u0, uint64_t u1) {
    const uint64_t r0 = u0 ? u0 - 1 : 0;
    return {r0, u1 > r0 ? u1 - r0 : 0, 0};
}

// the slice of table[0, n) that owns the positions [first, last]; one thread
KMAN_DEV TileSlice cut_slice(const uint64_t *table, uint64_t n, uint64_t first, uint64_t last) {
    return slice_of(upper_count(table, n, first), upper_count(table, n, last));
}
// the same with next = min(entry r0 + ns, limit), limit when the table ends with the slice
KMAN_DEV TileSlice cut_slice(const uint64_t *table, uint64_t n, uint64_t first, uint64_t last, uint64_t limit) {
    TileSlice s = cut_slice(table, n, first, last);
    s.next = s.r0 + s.ns < n ? umin64(table[s.r0 + s.ns], limit) : limit;
    return s;
}

// a cut slice as the kernel reads it: rs[0, ns) in LDS, or, big, in the table
struct SliceView {
    const uint64_t *rs;
    uint64_t ns, next;
    bool big;
    // entry i <= ns; entry ns: the first position after the slice
    KMAN_DEV uint64_t ent(uint64_t i) const { return i < ns ? rs[i] : next; }
};

// what stage_slice copies after the ns entries: nothing, s.next, or entry
// r0 + ns of a table of n + 1 entries (cut.hip's E, whose last entry is the total)
enum SliceTail { TAIL_NONE, TAIL_NEXT, TAIL_ENTRY };

// Block of NT threads: a slice of <= CAP entries goes to lds (CAP entries, CAP
// + 1 with a tail).  No barrier: the caller has one before lds is read.
template <int NT, int CAP, SliceTail TAIL = TAIL_NONE>
KMAN_DEV SliceView stage_slice(const uint64_t *__restrict__ table, const TileSlice &s, uint64_t *lds) {
    const bool big = s.ns > (uint64_t)CAP;
    if (!big) {
        if (TAIL == TAIL_NEXT) {
            for (uint32_t i = threadIdx.x; i <= (uint32_t)s.ns; i += NT)
                lds[i] = i < (uint32_t)s.ns ? table[s.r0 + i] : s.next;
        } else {
            const uint32_t n = (uint32_t)s.ns + (TAIL == TAIL_ENTRY ? 1u : 0u);
            for (uint32_t i = threadIdx.x; i < n; i += NT) lds[i] = table[s.r0 + i];
        }
    }
    return {big ? table + s.r0 : lds, s.ns, s.next, big};
}

// The owner walk of screen.hip and classify.hip.  The thread's EI consecutive
// windows start at positions p0 .. p0 + EI - 1 of the tile that starts at tb;
// bit j of `valid` says that window j counts.  The windows are cut into runs
// of one owner: the slice is searched again only where a window start passes
// nxt, the first position of the next owner.  Per run the walk keeps w, the
// number of valid windows, and an Acc (value-initialised at the run's start);
// add(acc, j) runs for every valid window, flush(acc, w, slot) for every
// finished run with w != 0 and an owner (u == 0: positions before the first
// record) whose slot lies in this round's window [round * CAP, round * CAP +
// CAP).  The slot is the owner's slice index on the LDS path (one round), and
// the offset of its first position in the tile on the global path (the owner
// that starts before the tile takes 0, which no other owner can have; tile
// size / CAP rounds), where the walk also notes the slot's record in srec.
template <int EI, int CAP, typename Acc, typename Add, typename Flush>
KMAN_DEV void owner_walk(const SliceView &v, uint64_t r0, uint64_t tb, uint64_t p0, uint32_t valid, int round,
                         uint64_t *srec, Add &&add, Flush &&flush) {
    const uint64_t slot0 = (uint64_t)round * CAP;
    uint64_t u = 0, nxt = 0;  // u: slice entries <= the current position; nxt: the position where that changes
    uint32_t w = 0;
    Acc acc{};
    auto finish = [&]() {
        if (w == 0 || u == 0) return;
        const uint64_t ri = u - 1;
        uint64_t key = ri;
        if (v.big) {
            const uint64_t st = v.rs[ri];
            key = st > tb ? st - tb : 0;
        }
        if (key >= slot0 && key - slot0 < (uint64_t)CAP) {
            const uint32_t slot = (uint32_t)(key - slot0);
            flush(acc, w, slot);
            if (v.big) srec[slot] = r0 + ri;  // (every writer of a slot stores the same record)
        }
    };
#pragma unroll
    for (int j = 0; j < EI; j++) {
        const uint64_t b = p0 + j;
        if (j == 0 || b >= nxt) {
            finish();
            w = 0;
            acc = Acc{};
            u = upper_count(v.rs, v.ns, b);
            nxt = u < v.ns ? v.rs[u] : ~0ull;
        }
        if ((valid >> j) & 1u) {
            w++;
            add(acc, j);
        }
    }
    finish();
}

}  // namespace
