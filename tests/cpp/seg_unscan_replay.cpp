// seg_unscan_replay.cpp -- the un-scan of photonlibos_amd/csrc/seg_unscan.h
// (photon_crc32c_copy_msg_iov_seg2_n / photon_crc64ecma_copy_msg_iov_seg2_n,
// DESIGN.md §4.13) on the host, stand-alone, for a build with
// -fsanitize=address,undefined: every array is heap memory of exactly its
// size, so a read or write outside an array shows. The entries that the walk
// does not store hold a canary: one that enters a result shows as a mismatch.
// Host only; nothing of the library is linked.
//
// argv[1]: the calls tests/test_seg_unscan_cpp.py writes, 64-bit little-endian
// words: the number of calls, then per call
//   nmsg, nsrc, ndst, has_size, has_seeds, seed32, seed64,
//   src_start[nmsg + 1], dst_start[nmsg + 1], src_len[nsrc], dst_len[ndst],
//   size[nmsg], seeds32[nmsg], seeds64[nmsg],
//   src_run32[nsrc], src_run64[nsrc], dst_run32[ndst], dst_run64[ndst],
//   src_want32[nsrc], src_want64[nsrc], dst_want32[ndst], dst_want64[ndst]
// (run: the oracle's running values where the walk stores them, a canary
// elsewhere; want: the oracle's per-segment CRCs). A message is a case.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "seg_unscan.h"

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

struct Call {
    uint64_t nmsg, nsrc, ndst, has_size, has_seeds, seed[2];
    const uint64_t *src_start, *dst_start, *src_len, *dst_len, *size, *seeds[2];
    const uint64_t *src_run[2], *dst_run[2], *src_want[2], *dst_want[2];
};

uint64_t g_runs = 0, g_bad = 0;

template <typename G>
void run_call(const Call& c, int w, const typename G::T* tab, uint32_t width) {
    typedef typename G::T T;
    uint64_t* src_start = exact<uint64_t>(c.src_start, c.nmsg + 1);
    uint64_t* dst_start = exact<uint64_t>(c.dst_start, c.nmsg + 1);
    uint64_t* src_len = exact<uint64_t>(c.src_len, c.nsrc);
    uint64_t* dst_len = exact<uint64_t>(c.dst_len, c.ndst);
    uint64_t* size = c.has_size ? exact<uint64_t>(c.size, c.nmsg) : nullptr;
    T* seeds = c.has_seeds ? exact<T>(c.seeds[w], c.nmsg) : nullptr;
    T* src_seg = exact<T>(c.src_run[w], c.nsrc);
    T* dst_seg = exact<T>(c.dst_run[w], c.ndst);
    for (uint64_t m = 0; m < c.nmsg; ++m)
        unscan_replay_msg<G>(src_len, src_start, dst_len, dst_start, m, size, (T)c.seed[w], seeds, src_seg, dst_seg,
                             tab, width);
    ++g_runs;
    auto compare = [&](const char* side, const T* got, const uint64_t* want, uint64_t n) {
        for (uint64_t s = 0; s < n; ++s)
            if (got[s] != (T)want[s]) {
                if (!g_bad++)
                    fprintf(stderr, "crc%d width %u %s entry %llu of %llu: %llx, want %llx\n", w ? 64 : 32, width, side,
                            (unsigned long long)s, (unsigned long long)n, (unsigned long long)got[s],
                            (unsigned long long)want[s]);
            }
    };
    compare("src", src_seg, c.src_want[w], c.nsrc);
    compare("dst", dst_seg, c.dst_want[w], c.ndst);
    free(src_start), free(dst_start), free(src_len), free(dst_len), free(size), free(seeds), free(src_seg),
        free(dst_seg);
}

}  // namespace

int main(int argc, char** argv) {
    if (argc != 2) return fprintf(stderr, "usage: %s cases.bin\n", argv[0]), 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return perror(argv[1]), 2;
    fseek(f, 0, SEEK_END);
    const long bytes = ftell(f);
    fseek(f, 0, SEEK_SET);
    std::vector<uint64_t> words((size_t)bytes / 8);
    if (bytes % 8 || fread(words.data(), 8, words.size(), f) != words.size()) return fprintf(stderr, "short file\n"), 2;
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
    const uint64_t ncalls = *take(1);
    uint64_t ncases = 0;
    for (uint64_t k = 0; k < ncalls; ++k) {
        const uint64_t* h = take(7);
        Call c = {};
        c.nmsg = h[0], c.nsrc = h[1], c.ndst = h[2], c.has_size = h[3], c.has_seeds = h[4];
        c.seed[0] = h[5], c.seed[1] = h[6];
        c.src_start = take(c.nmsg + 1), c.dst_start = take(c.nmsg + 1);
        c.src_len = take(c.nsrc), c.dst_len = take(c.ndst);
        c.size = take(c.nmsg);
        c.seeds[0] = take(c.nmsg), c.seeds[1] = take(c.nmsg);
        c.src_run[0] = take(c.nsrc), c.src_run[1] = take(c.nsrc);
        c.dst_run[0] = take(c.ndst), c.dst_run[1] = take(c.ndst);
        c.src_want[0] = take(c.nsrc), c.src_want[1] = take(c.nsrc);
        c.dst_want[0] = take(c.ndst), c.dst_want[1] = take(c.ndst);
        ncases += c.nmsg;
        // the kernel's step width, and two that cut the sides elsewhere
        for (uint32_t width : {kUnscanStep, 1u, 7u}) {
            run_call<Gf32>(c, 0, tab32, width);
            run_call<Gf64>(c, 1, tab64, width);
        }
    }
    if (at != words.size()) return fprintf(stderr, "trailing words\n"), 2;
    printf("seg_unscan_replay: %llu cases, %llu runs, %llu mismatches\n", (unsigned long long)ncases,
           (unsigned long long)g_runs, (unsigned long long)g_bad);
    return g_bad ? 1 : 0;
}
