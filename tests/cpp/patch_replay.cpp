// patch_replay.cpp -- photonlibos_amd/csrc/patch_crc.h (photon_crc32c_patch_n /
// photon_crc64ecma_patch_n) on the host, stand-alone, for a
// build with -fsanitize=address,undefined: every array is heap memory of
// exactly its size, so a read or write outside an array shows. Host only;
// nothing of the library is linked.
//
// argv[1]: the cases tests/test_patch_cpp.py writes (the fuzz of
// tests/test_patch_abi.py with the oracle's words, and its large tails),
// 64-bit little-endian words: the number of cases, then per case
//   nwrites, ntgt, has_start,
//   delta32[nwrites], delta64[nwrites], tail[nwrites], tgt_start[ntgt + 1] if has_start,
//   in32[ntgt], in64[ntgt], want32[ntgt], want64[ntgt].
// Each case also runs in place (out == in) and, with a tgt_start, with
// tgt_start arrays that break the rules: the values are unspecified then, the
// accesses are not.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "patch_crc.h"

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
    uint64_t nwrites, ntgt, has_start;
    const uint64_t *delta[2], *tail, *start, *in[2], *want[2];
};

uint64_t g_runs = 0, g_bad = 0;

template <typename G>
void run_case(const Case& c, int w, const typename G::T* tab, const uint64_t* start_words, bool compare, uint32_t nt,
              bool in_place) {
    typedef typename G::T T;
    T* delta = exact<T>(c.delta[w], c.nwrites);
    uint64_t* tail = exact<uint64_t>(c.tail, c.nwrites);
    uint64_t* start = start_words ? exact<uint64_t>(start_words, c.ntgt + 1) : nullptr;
    T* in = exact<T>(c.in[w], c.ntgt);
    T* out = in_place ? in : static_cast<T*>(malloc(c.ntgt ? c.ntgt * sizeof(T) : 1));
    if (!in_place) memset(out, 0xA5, c.ntgt * sizeof(T));
    patch_replay<G>(delta, tail, c.nwrites, start, c.ntgt, in, out, nt, tab);
    ++g_runs;
    if (compare)
        for (uint64_t m = 0; m < c.ntgt; ++m)
            if (out[m] != (T)c.want[w][m]) {
                if (!g_bad++)
                    fprintf(stderr, "crc%d nt %u target %llu of %llu: %llx, want %llx\n", w ? 64 : 32, nt,
                            (unsigned long long)m, (unsigned long long)c.ntgt, (unsigned long long)out[m],
                            (unsigned long long)c.want[w][m]);
                break;
            }
    if (!in_place) free(out);
    free(delta), free(tail), free(start), free(in);
}

template <typename G>
void run_width(const Case& c, int w, const typename G::T* tab, uint64_t k) {
    static const uint32_t kThreads[] = {1, 3, 7, 64, 256};
    for (uint32_t nt : kThreads) run_case<G>(c, w, tab, c.start, true, nt, (k + nt) % 2 != 0);
    if (!c.has_start) return;
    // tgt_start that breaks its rules: reversed, not from 0, beyond nwrites, all equal
    std::vector<uint64_t> bad(c.start, c.start + c.ntgt + 1);
    for (int variant = 0; variant < 4; ++variant) {
        for (uint64_t m = 0; m <= c.ntgt; ++m)
            bad[m] = variant == 0   ? c.start[c.ntgt - m]
                     : variant == 1 ? c.start[m] + 5
                     : variant == 2 ? c.start[m] * 1000 + (m == c.ntgt ? ~0ull >> 1 : 0)
                                    : c.nwrites / 2;
        run_case<G>(c, w, tab, bad.data(), false, variant == 3 ? 7 : 64, variant & 1);
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
    for (uint64_t k = 0; k < ncases; ++k) {
        const uint64_t* h = take(3);
        Case c = {h[0], h[1], h[2], {nullptr, nullptr}, nullptr, nullptr, {nullptr, nullptr}, {nullptr, nullptr}};
        c.delta[0] = take(c.nwrites), c.delta[1] = take(c.nwrites);
        c.tail = take(c.nwrites);
        c.start = c.has_start ? take(c.ntgt + 1) : nullptr;
        c.in[0] = take(c.ntgt), c.in[1] = take(c.ntgt);
        c.want[0] = take(c.ntgt), c.want[1] = take(c.ntgt);
        run_width<Gf32>(c, 0, tab32, k);
        run_width<Gf64>(c, 1, tab64, k);
    }
    if (at != words.size()) return fprintf(stderr, "trailing words\n"), 2;
    printf("patch_replay: %llu cases, %llu runs, %llu mismatches\n", (unsigned long long)ncases,
           (unsigned long long)g_runs, (unsigned long long)g_bad);
    return g_bad ? 1 : 0;
}
