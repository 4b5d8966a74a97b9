// swar.h — byte tests on packed words and bit-mask helpers that the two text
// parsers share (parse.hip, fastq.hip): a thread's chunk of the text lives in
// registers as 32-bit words and is reduced to 64-bit masks, bit i = byte i.
#pragma once
#include "common.h"

namespace {

KMAN_DEV bool is_term(uint32_t c) { return c == '\n' || c == '\r'; }
// Python str.isspace() over ASCII: what str.rstrip() strips.
KMAN_DEV bool py_space(uint32_t c) { return c == ' ' || (c >= 9 && c <= 13) || (c >= 0x1c && c <= 0x1f); }

// byte i of N packed words (indexed at compile time only, so w stays in registers)
template <int N>
KMAN_DEV uint32_t byte_at(const uint32_t (&w)[N], int i) {
    return (w[i >> 2] >> (8 * (i & 3))) & 0xffu;
}

// SWAR byte tests on 4 packed bytes: 0x80 in every byte that passes
KMAN_DEV uint32_t zero_bytes(uint32_t t) { return ~(((t & 0x7f7f7f7fu) + 0x7f7f7f7fu) | t | 0x7f7f7f7fu); }
KMAN_DEV uint32_t eq_bytes(uint32_t w, uint32_t c) { return zero_bytes(w ^ (c * 0x01010101u)); }
// the 0x80 bits of four bytes -> a 4-bit mask
KMAN_DEV uint32_t hibits4(uint32_t m) {
    m >>= 7;
    return (m | (m >> 7) | (m >> 14) | (m >> 21)) & 0xfu;
}
// base codes of four bytes (A/a 0, C/c 1, G/g 2, T/t 3, else 4): (c >> 1) & 3
// maps A C T G to 0 1 2 3, x ^ (x >> 1) swaps the last two
KMAN_DEV uint32_t codes4(uint32_t w) {
    const uint32_t x = (w >> 1) & 0x03030303u;
    const uint32_t code = x ^ ((x >> 1) & 0x01010101u);
    const uint32_t y = w | 0x20202020u;
    const uint32_t ok = eq_bytes(y, 'a') | eq_bytes(y, 'c') | eq_bytes(y, 'g') | eq_bytes(y, 't');
    return (code & ((ok >> 7) * 3u)) | ((~ok & 0x80808080u) >> 5);
}
KMAN_DEV uint64_t bits_from(int i) { return i >= 64 ? 0ull : (~0ull << i); }
KMAN_DEV uint64_t bits_below(int i) { return i >= 64 ? ~0ull : ((1ull << i) - 1); }

}  // namespace
