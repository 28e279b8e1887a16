// scan_parts_replay.cpp -- the three steps of photonlibos_amd/csrc/scan_parts.h
// (photon_crc32c_scan_parts_n / photon_crc64ecma_scan_parts_n, DESIGN.md
// §4.11) on the host, stand-alone, for a build with
// -fsanitize=address,undefined: every array is heap memory of exactly its
// size, and the workspace is filled with 0xA5 and never cleared, so a read or
// write outside an array, or a workspace word read before it was written,
// shows. Host only; nothing of the library is linked.
//
// argv[1]: the cases tests/test_scan_parts_cpp.py writes (the boundary fuzz of
// tests/test_scan_parts_abi.py with the oracle's running words), 64-bit
// little-endian words: the number of cases, then per case
//   nobj, nparts, per_object, seed32, seed64,
//   obj_start[nobj + 1], len[nparts], crc32[nparts], crc64[nparts],
//   seeds32[nobj], seeds64[nobj], want32[nparts], want64[nparts], end[nparts]
// (want: from seeds[m] if per_object, else from seed32 / seed64).
// Each case also runs with obj_start arrays that break the rules: the values
// are unspecified then, the accesses are not.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "scan_parts.h"

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
    uint64_t nobj, nparts, per_object, seed[2];
    const uint64_t *start, *len, *crc[2], *seeds[2], *want[2], *end;
};

uint64_t g_runs = 0, g_bad = 0;

template <typename G>
void run_case(const Case& c, int w, const typename G::T* tab, const uint64_t* start_words, bool compare,
              uint32_t tile, uint32_t nt, bool with_end) {
    typedef typename G::T T;
    T* crc = exact<T>(c.crc[w], c.nparts);
    uint64_t* len = exact<uint64_t>(c.len, c.nparts);
    uint64_t* start = start_words ? exact<uint64_t>(start_words, c.nobj + 1) : nullptr;
    T* seeds = c.per_object ? exact<T>(c.seeds[w], c.nobj) : nullptr;
    T* run = static_cast<T*>(malloc(c.nparts * sizeof(T)));
    uint64_t* end = with_end ? static_cast<uint64_t*>(malloc(c.nparts * 8)) : nullptr;
    const uint64_t words = scan_work_words(c.nparts, tile);
    uint64_t* work = static_cast<uint64_t*>(malloc(words * 8));
    memset(run, 0xA5, c.nparts * sizeof(T));
    if (end) memset(end, 0xA5, c.nparts * 8);
    memset(work, 0xA5, words * 8);
    const ScanIn<T> in = {crc, len, start, start ? c.nobj : 1, c.nparts, (T)c.seed[w], seeds};
    scan_replay<G>(in, tile, nt, tab, work, run, end);
    ++g_runs;
    if (compare)
        for (uint64_t s = 0; s < c.nparts; ++s)
            if (run[s] != (T)c.want[w][s] || (end && end[s] != c.end[s])) {
                if (!g_bad++)
                    fprintf(stderr, "crc%d tile %u nt %u part %llu of %llu: %llx, want %llx\n", w ? 64 : 32, tile, nt,
                            (unsigned long long)s, (unsigned long long)c.nparts, (unsigned long long)run[s],
                            (unsigned long long)c.want[w][s]);
                break;
            }
    free(crc), free(len), free(start), free(seeds), free(run), free(end), free(work);
}

template <typename G>
void run_width(const Case& c, int w, const typename G::T* tab, uint64_t k) {
    static const uint32_t kThreads[] = {1, 3, 7, 64, 256};
    for (uint32_t tile : {64u, 128u})
        for (uint32_t nt : kThreads) run_case<G>(c, w, tab, c.start, true, tile, nt, (k + nt) % 3 != 0);
    if (c.nobj == 1) run_case<G>(c, w, tab, nullptr, true, 64, 64, true);  // a null obj_start: one object
    // obj_start that breaks its rules: reversed, not from 0, beyond nparts, all equal
    std::vector<uint64_t> bad(c.start, c.start + c.nobj + 1);
    for (int variant = 0; variant < 4; ++variant) {
        for (uint64_t m = 0; m <= c.nobj; ++m)
            bad[m] = variant == 0   ? c.start[c.nobj - m]
                     : variant == 1 ? c.start[m] + 5
                     : variant == 2 ? c.start[m] * 1000 + (m == c.nobj ? ~0ull >> 1 : 0)
                                    : c.nparts / 2;
        run_case<G>(c, w, tab, bad.data(), false, 64, variant == 3 ? 7 : 64, true);
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
        const uint64_t* h = take(5);
        Case c = {h[0], h[1], h[2], {h[3], h[4]}, nullptr, nullptr, {nullptr, nullptr}, {nullptr, nullptr},
                  {nullptr, nullptr}, nullptr};
        c.start = take(c.nobj + 1);
        c.len = take(c.nparts);
        c.crc[0] = take(c.nparts), c.crc[1] = take(c.nparts);
        c.seeds[0] = take(c.nobj), c.seeds[1] = take(c.nobj);
        c.want[0] = take(c.nparts), c.want[1] = take(c.nparts);
        c.end = take(c.nparts);
        run_width<Gf32>(c, 0, tab32, k);
        run_width<Gf64>(c, 1, tab64, k);
    }
    if (at != words.size()) return fprintf(stderr, "trailing words\n"), 2;
    printf("scan_parts_replay: %llu cases, %llu runs, %llu mismatches\n", (unsigned long long)ncases,
           (unsigned long long)g_runs, (unsigned long long)g_bad);
    return g_bad ? 1 : 0;
}
