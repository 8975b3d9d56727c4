// Stand-alone check of speq_amd/csrc/ax_phase1.hpp (tests/test_ax_phase1_cpu.py builds it with plain g++ and runs it):
// includes nothing but that header, so the formulas under test are the kernel's own.
//   mismatch  axp_first_mismatch against a base-by-base loop over byte arrays: every text offset s5 0..31, every read
//             shift 0..15, a mismatch at every base 0..159 and none, pairs of mismatches, random bases past cl
// Prints "mismatch cases=<n> fail=<n>", and the first failures on stderr. Exit status 1 on a failure.
#include <cstdint>
#include <cstdio>

#include "ax_phase1.hpp"

using namespace speq_dev;

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd() {  // xorshift64*
    rng_state ^= rng_state >> 12;
    rng_state ^= rng_state << 25;
    rng_state ^= rng_state >> 27;
    return (uint32_t)((rng_state * 0x2545F4914F6CDD1Dull) >> 32);
}

// ---- first mismatch -------------------------------------------------------------------------------------------------
constexpr uint32_t TB = 16u * (AXP_CMPD + 2u);  // text bases in T
constexpr uint32_t RB = 16u * (AXP_CMPD + 1u);  // read bases in rw

static void pack(const uint8_t* b, uint32_t n, uint32_t* w) {  // base i at bits 2 (i % 16) of dword i / 16
    for (uint32_t i = 0; i < n / 16u; ++i) w[i] = 0;
    for (uint32_t i = 0; i < n; ++i) w[i / 16u] |= (uint32_t)(b[i] & 3u) << (2u * (i % 16u));
}
static uint32_t by_base(const uint8_t* tx, const uint8_t* rd, uint32_t s5, uint32_t rs, uint32_t cl) {
    for (uint32_t b = 0; b < cl; ++b)
        if (tx[s5 + b] != rd[rs + b]) return b;
    return cl;
}

static uint64_t mm_cases = 0, mm_fail = 0;
static void mm_one(const uint8_t* tx, const uint8_t* rd, uint32_t s5, uint32_t rs, uint32_t cl) {
    uint32_t T[AXP_CMPD + 2], rw[AXP_CMPD + 1];
    pack(tx, TB, T);
    pack(rd, RB, rw);
    const uint32_t got = axp_first_mismatch(T, rw, s5, 2u * rs, cl), exp = by_base(tx, rd, s5, rs, cl);
    ++mm_cases;
    if (got != exp && mm_fail++ < 10) fprintf(stderr, "mismatch: s5=%u shift=%u cl=%u got=%u expected=%u\n", s5, rs, cl, got, exp);
}
// a read equal to the text over 160 bases from (s5, rs), random elsewhere; then the bases at m0 and m1 (>= 160: none)
// replaced by another base, and the bases from `wild` on by random ones
static void mm_build(const uint8_t* tx, uint8_t* rd, uint32_t s5, uint32_t rs, uint32_t m0, uint32_t m1, uint32_t wild) {
    for (uint32_t i = 0; i < RB; ++i) rd[i] = (uint8_t)(rnd() & 3u);
    for (uint32_t b = 0; b < 160u && b < wild; ++b) rd[rs + b] = tx[s5 + b];
    if (m0 < 160u) rd[rs + m0] = (uint8_t)((tx[s5 + m0] + 1u + rnd() % 3u) & 3u);
    if (m1 < 160u) rd[rs + m1] = (uint8_t)((tx[s5 + m1] + 1u + rnd() % 3u) & 3u);
}
static void check_mismatch() {
    uint8_t tx[TB], rd[RB];
    for (uint32_t s5 = 0; s5 < 32u; ++s5)
        for (uint32_t rs = 0; rs < 16u; ++rs) {
            for (uint32_t i = 0; i < TB; ++i) tx[i] = (uint8_t)(rnd() & 3u);
            for (uint32_t m = 0; m <= 160u; ++m) {  // (160: no mismatch)
                mm_build(tx, rd, s5, rs, m, 160u, 160u);
                mm_one(tx, rd, s5, rs, 160u);                      // the whole compare
                if (m >= 1u) mm_one(tx, rd, s5, rs, m);            // the mismatch is the first base past cl
                if (m < 160u) mm_one(tx, rd, s5, rs, m + 1u);      // ... the last base before cl
                const uint32_t cl = 1u + rnd() % 160u;
                mm_one(tx, rd, s5, rs, cl);
                mm_build(tx, rd, s5, rs, m, 160u, cl);             // arbitrary words past cl
                mm_one(tx, rd, s5, rs, cl);
            }
            for (uint32_t t = 0; t < 64u; ++t) {  // two mismatches: in one dword, in neighbours, far apart
                const uint32_t a = rnd() % 160u;
                const uint32_t gap = t < 16u ? 1u + rnd() % 3u : (t < 32u ? 1u + rnd() % 31u : 1u + rnd() % 159u);
                const uint32_t b = a + gap < 160u ? a + gap : (a + 159u) % 160u;
                mm_build(tx, rd, s5, rs, a, b, 160u);
                mm_one(tx, rd, s5, rs, 160u);
                mm_one(tx, rd, s5, rs, 1u + rnd() % 160u);
            }
        }
    printf("mismatch cases=%llu fail=%llu\n", (unsigned long long)mm_cases, (unsigned long long)mm_fail);
}

int main() {
    check_mismatch();
    return mm_fail ? 1 : 0;
}
