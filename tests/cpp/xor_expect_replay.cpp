// xor_expect_replay.cpp -- photonlibos_amd/csrc/xor_expect.h
// (photon_crc32c_xor_expect_n / photon_crc64ecma_xor_expect_n)
// on the host, stand-alone, for a build with -fsanitize=address,undefined:
// every array is heap memory of exactly its size, so a read or write outside
// an array shows. Host only; nothing of the library is linked.
//
// argv[1]: the cases tests/test_xor_expect_cpp.py writes (the fuzz of
// tests/test_xor_expect_abi.py with the oracle's words, and its large
// lengths), 64-bit little-endian words: the number of cases, then per case
//   count, ncrc, has_start, k, has_len, nbytes, seed32, seed64,
//   crc32[ncrc], crc64[ncrc], grp_start[count + 1] if has_start, len[count] if has_len,
//   want32[count], want64[count].
// With a grp_start each case also runs with grp_start arrays that break the
// rules: the values are unspecified then, the accesses are not.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "xor_expect.h"

using namespace pcrc;

namespace {

template <typename G>
void power_table(typename G::T x8, typename G::T tab[64]) {
    tab[0] = x8;  // x^(8 * 2^i)
    for (int i = 1; i < 64; ++i) tab[i] = G::mul(tab[i - 1], tab[i - 1]);
}

template <typename T>
T* exact(const uint64_t* src, uint64_t n) {  // n words on the heap, no slack
    T* p = static_cast<T*>(malloc(n ? n * sizeof(T) : 1));
    for (uint64_t i = 0; i < n; ++i) p[i] = (T)src[i];
    return p;
}

struct Case {
    uint64_t count, ncrc, has_start, k, has_len, nbytes, seed[2];
    const uint64_t *crc[2], *start, *len, *want[2];
};

uint64_t g_runs = 0, g_bad = 0;

template <typename G>
void run_case(const Case& c, int w, const typename G::T* tab, const uint64_t* start_words, bool compare) {
    typedef typename G::T T;
    T* crc = exact<T>(c.crc[w], c.ncrc);
    uint64_t* start = start_words ? exact<uint64_t>(start_words, c.count + 1) : nullptr;
    uint64_t* len = c.has_len ? exact<uint64_t>(c.len, c.count) : nullptr;
    T* want = static_cast<T*>(malloc(c.count ? c.count * sizeof(T) : 1));
    memset(want, 0xA5, c.count * sizeof(T));
    const T inv = w ? ~(T)0 : (T)0;
    xor_expect_replay<G>(crc, c.ncrc, start, (uint32_t)c.k, len, c.nbytes, c.count, (T)c.seed[w], inv, want, tab);
    ++g_runs;
    if (compare)
        for (uint64_t s = 0; s < c.count; ++s)
            if (want[s] != (T)c.want[w][s]) {
                if (!g_bad++)
                    fprintf(stderr, "crc%d stripe %llu of %llu: %llx, want %llx\n", w ? 64 : 32, (unsigned long long)s,
                            (unsigned long long)c.count, (unsigned long long)want[s],
                            (unsigned long long)c.want[w][s]);
                break;
            }
    free(crc), free(start), free(len), free(want);
}

template <typename G>
void run_width(const Case& c, int w, const typename G::T* tab) {
    run_case<G>(c, w, tab, c.start, true);
    if (!c.has_start) return;
    // grp_start that breaks its rules: reversed, not from 0, beyond ncrc, all equal
    std::vector<uint64_t> bad(c.start, c.start + c.count + 1);
    for (int variant = 0; variant < 4; ++variant) {
        for (uint64_t m = 0; m <= c.count; ++m)
            bad[m] = variant == 0   ? c.start[c.count - m]
                     : variant == 1 ? c.start[m] + 5
                     : variant == 2 ? c.start[m] * 1000 + (m == c.count ? ~0ull >> 1 : 0)
                                    : c.ncrc / 2;
        run_case<G>(c, w, tab, bad.data(), false);
    }
}

}  // namespace

int main(int argc, char** argv) {
    if (argc != 2) return fprintf(stderr, "usage: %s cases.bin\n", argv[0]), 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return perror(argv[1]), 2;
    fseek(f, 0, SEEK_END);
    const long size = ftell(f);
    fseek(f, 0, SEEK_SET);
    std::vector<uint64_t> words((size_t)size / 8);
    if (size % 8 || fread(words.data(), 8, words.size(), f) != words.size()) return fprintf(stderr, "short file\n"), 2;
    fclose(f);

    uint32_t tab32[64];
    uint64_t tab64[64];
    power_table<Gf32>(xpow(8), tab32);
    power_table<Gf64>(xpow64(8), tab64);

    size_t at = 0;
    auto take = [&](uint64_t n) {
        const uint64_t* p = words.data() + at;
        at += n;
        if (at > words.size()) exit((fprintf(stderr, "truncated file\n"), 2));
        return p;
    };
    const uint64_t ncases = *take(1);
    for (uint64_t i = 0; i < ncases; ++i) {
        const uint64_t* h = take(8);
        Case c = {h[0], h[1], h[2], h[3], h[4], h[5], {h[6], h[7]}, {nullptr, nullptr}, nullptr, nullptr,
                  {nullptr, nullptr}};
        c.crc[0] = take(c.ncrc), c.crc[1] = take(c.ncrc);
        c.start = c.has_start ? take(c.count + 1) : nullptr;
        c.len = c.has_len ? take(c.count) : nullptr;
        c.want[0] = take(c.count), c.want[1] = take(c.count);
        run_width<Gf32>(c, 0, tab32);
        run_width<Gf64>(c, 1, tab64);
    }
    if (at != words.size()) return fprintf(stderr, "trailing words\n"), 2;
    printf("xor_expect_replay: %llu cases, %llu runs, %llu mismatches\n", (unsigned long long)ncases,
           (unsigned long long)g_runs, (unsigned long long)g_bad);
    return g_bad ? 1 : 0;
}
