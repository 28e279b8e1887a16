// window_finish_replay.cpp -- the finish of the windowed copy + CRC
// (photonlibos_amd/csrc/window_finish.h, photon_crc32c_copy_msg_iov_window_n /
// photon_crc64ecma_copy_msg_iov_window_n) on the host,
// stand-alone, also built with -fsanitize=address,undefined: every array the
// replay touches is heap memory of exactly its size.
//
// Linked with crc32c_cpu.cpp and crc64_cpu.cpp: the CPU engines (crc32c_sw,
// crc64ecma_sw) play the kernel's checksum unit in a host model of the walk
// (walk_model: the pieces in front of, inside and behind the window, chained
// from seed 0, the running value stored at every segment end and at the two
// window edges; a canary in every entry beforehand), and they compute the
// expected results directly: every whole segment from seed 0, the window's
// bytes from the message's seed, and k from 128-bit arithmetic.
//
// No input: the cases are made here (cases()). Prints
//   window_finish_replay: <cases> cases, <runs> runs, <mismatches> mismatches
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include <photon/common/checksum/crc32c.h>
#include <photon/common/checksum/crc64ecma.h>

#include "window_finish.h"

using namespace pcrc;

namespace {

const uint64_t kAll = ~0ull;

struct E32 : Gf32 {
    static T crc(const uint8_t* p, size_t n, T seed) { return crc32c_sw(p, n, seed); }
    static constexpr T kCanary = 0xA5A5A5A5u;
    static constexpr int kBits = 32;
};
struct E64 : Gf64 {
    static T crc(const uint8_t* p, size_t n, T seed) { return crc64ecma_sw(p, n, seed); }
    static constexpr T kCanary = 0xA5A5A5A5A5A5A5A5ull;
    static constexpr int kBits = 64;
};

template <typename G>
void power_table(typename G::T x8, typename G::T tab[64]) {
    tab[0] = x8;  // x^(8 * 2^i)
    for (int i = 1; i < 64; ++i) tab[i] = G::mul(tab[i - 1], tab[i - 1]);
}

template <typename T>
T* exact(const std::vector<T>& v) {  // on the heap, no slack
    T* p = static_cast<T*>(malloc(v.size() ? v.size() * sizeof(T) : 1));
    if (!v.empty()) memcpy(p, v.data(), v.size() * sizeof(T));
    return p;
}

uint64_t splitmix(uint64_t* s) {
    uint64_t z = (*s += 0x9e3779b97f4a7c15ull);
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
}

struct Case {
    std::vector<uint64_t> src, dst;  // segment lengths
    uint64_t skip, size;
    uint64_t seed;                   // CRC-32C takes its low half
};

// The walk of one message over `bytes` (the source stream) as the kernel runs
// it, with the CPU engine as its checksum unit: the pieces in front of the
// window, the window's (cut by both sides' segments and the cap), the pieces
// behind it. seg: one entry per source segment; work: two words.
template <typename E>
void walk_model(const Case& c, const uint8_t* bytes, typename E::T* seg, uint64_t* work) {
    typename E::T acc = 0;
    size_t si = 0, di = 0;
    uint64_t srem = c.src.empty() ? 0 : c.src[0];
    const uint8_t* p = bytes;
    auto piece = [&](uint64_t n) {
        acc = E::crc(p, n, acc);
        p += n, srem -= n;
    };
    auto seg_end = [&] {
        if (!srem) {
            seg[si] = acc;
            if (++si < c.src.size()) srem = c.src[si];
        }
    };
    auto skim = [&](uint64_t cnt) {
        while (cnt && si < c.src.size()) {
            const uint64_t n = srem < cnt ? srem : cnt;
            cnt -= n;
            piece(n);
            seg_end();
        }
    };
    skim(c.skip);
    work[0] = acc;
    uint64_t left = c.size, drem = c.dst.empty() ? 0 : c.dst[0];
    while (left && si < c.src.size() && di < c.dst.size()) {
        uint64_t n = srem < drem ? srem : drem;
        n = n < left ? n : left;
        piece(n);
        drem -= n, left -= n;
        if (!left) break;
        seg_end();
        if (!drem && ++di < c.dst.size()) drem = c.dst[di];
    }
    work[1] = acc;
    skim(kAll);
}

std::vector<Case> cases() {
    std::vector<Case> out;
    typedef std::vector<uint64_t> V;
    const std::vector<V> srcs = {
        {100, 200, 300},        // L = 600: boundaries at 100 and 300
        {0, 0, 50, 70},         // zero-length segments first
        {50, 70, 0, 0},         // last
        {50, 0, 0, 70},         // adjacent, in the middle
        {0, 17, 0, 0, 33, 0},   // everywhere
        {1},
        {},
        {0, 0},
    };
    const std::vector<V> dsts = {
        {1000},                 // room for everything
        {30, 40},               // D = 70, smaller than most windows
        {},                     // no destination segments
        {0, 0, 500, 0},         // zero-length first, adjacent and last
        {0, 25, 0, 0, 35, 0},
        {0, 0, 0},              // D = 0
    };
    uint64_t sd = 0x5EED0057ull;
    for (const V& s : srcs) {
        uint64_t L = 0;
        for (uint64_t n : s) L += n;
        // 0, 1, inside a segment, on the segment boundaries, L - 1, L, beyond L, ~0
        V skips = {0, 1, L / 2 + 1, L ? L - 1 : 0, L, L + 1, L + 1000, 1ull << 63, kAll - 1, kAll};
        uint64_t run = 0;
        for (uint64_t n : s) skips.push_back(run += n);
        for (uint64_t skip : skips) {
            // 0, 1, unlimited, larger than what is left, skip + size past 2^64
            const V sizes = {0, 1, 7, L / 3, L, L + 5, kAll, kAll - 10, kAll - skip, kAll - skip + 1, 1ull << 63};
            for (uint64_t size : sizes)
                for (const V& d : dsts)
                    out.push_back(Case{s, d, skip, size, out.size() % 3 ? splitmix(&sd) : 0});
        }
    }
    // more segments than one step of the finish (64), on both sides, lengths 0..8
    for (size_t ns : {63, 64, 65, 129, 200})
        for (size_t nd : {1, 64, 130}) {
            Case c;
            uint64_t L = 0;
            for (size_t i = 0; i < ns; ++i) c.src.push_back(splitmix(&sd) % 9), L += c.src.back();
            for (size_t i = 0; i < nd; ++i) c.dst.push_back(splitmix(&sd) % (nd == 1 ? 2000 : 9));
            for (int r = 0; r < 6; ++r) {
                c.skip = r == 0 ? 0 : splitmix(&sd) % (L + 2);
                c.size = r == 1 ? kAll : splitmix(&sd) % (L + 2);
                c.seed = splitmix(&sd);
                out.push_back(c);
            }
        }
    return out;
}

uint64_t g_runs = 0, g_bad = 0;

void bad(const char* what, int bits, uint32_t width, size_t m, unsigned long long got, unsigned long long want) {
    if (!g_bad++) fprintf(stderr, "crc%d width %u message %zu %s: %llx, want %llx\n", bits, width, m, what, got, want);
}

// One call with every case as a message. mode: 0 = per-message seeds, skip and
// size arrays; 1 = seed0 alone and no size array (the cases whose size is
// unlimited); 2 = no skip array (the cases whose skip is 0), no copied.
template <typename E>
void run_call(const std::vector<Case>& all, int mode, uint32_t width, const typename E::T* tab) {
    typedef typename E::T T;
    std::vector<Case> cs;
    for (const Case& c : all)
        if (mode == 0 || (mode == 1 && c.size == kAll) || (mode == 2 && c.skip == 0)) cs.push_back(c);
    const T seed0 = (T)0xFEEDC0DE5EED0001ull;
    std::vector<uint64_t> src_start{0}, dst_start{0}, src_len, dst_len, skip, size, work, want_k;
    std::vector<T> seeds, seg, want_seg, want_out;
    uint64_t sd = 0xB17E5ull + mode;
    for (const Case& c : cs) {
        unsigned __int128 L = 0, D = 0;
        for (uint64_t n : c.src) L += n;
        for (uint64_t n : c.dst) D += n;
        std::vector<uint8_t> bytes((size_t)L + 1);
        for (uint8_t& b : bytes) b = (uint8_t)splitmix(&sd);
        // the model of the walk
        std::vector<T> s(c.src.size(), E::kCanary);
        uint64_t w[2] = {0xA5A5A5A5A5A5A5A5ull, 0xA5A5A5A5A5A5A5A5ull};
        walk_model<E>(c, bytes.data(), s.data(), w);
        seg.insert(seg.end(), s.begin(), s.end());
        work.push_back(w[0]), work.push_back(w[1]);
        // what the call must return, computed directly
        const unsigned __int128 a = c.skip < L ? c.skip : L;
        unsigned __int128 k = c.size < D ? c.size : D;
        k = k < L - a ? k : L - a;
        const T seed = mode == 1 ? seed0 : (T)c.seed;
        const uint8_t* p = bytes.data();
        for (uint64_t n : c.src) want_seg.push_back(E::crc(p, n, 0)), p += n;
        want_out.push_back(E::crc(bytes.data() + (size_t)a, (size_t)k, seed));
        want_k.push_back((uint64_t)k);
        src_len.insert(src_len.end(), c.src.begin(), c.src.end());
        dst_len.insert(dst_len.end(), c.dst.begin(), c.dst.end());
        src_start.push_back(src_len.size()), dst_start.push_back(dst_len.size());
        skip.push_back(c.skip), size.push_back(c.size), seeds.push_back((T)c.seed);
    }
    const size_t nmsg = cs.size();
    uint64_t *h_ss = exact(src_start), *h_ds = exact(dst_start), *h_sl = exact(src_len), *h_dl = exact(dst_len);
    uint64_t* h_skip = mode == 2 ? nullptr : exact(skip);
    uint64_t* h_size = mode == 1 ? nullptr : exact(size);
    T* h_seeds = mode == 1 ? nullptr : exact(seeds);
    T* h_seg = exact(seg);
    uint64_t* h_work = exact(work);
    T* h_out = exact(std::vector<T>(nmsg, E::kCanary));
    uint64_t* h_copied = mode == 2 ? nullptr : exact(std::vector<uint64_t>(nmsg, 0xA5A5A5A5A5A5A5A5ull));
    for (size_t m = 0; m < nmsg; ++m)
        window_replay_msg<E>(h_sl, h_ss, h_dl, h_ds, m, h_skip, h_size, seed0, h_seeds, h_seg, h_work, h_out, h_copied,
                             tab, width);
    ++g_runs;
    for (size_t m = 0; m < nmsg; ++m) {
        if (h_out[m] != want_out[m]) bad("window crc", E::kBits, width, m, h_out[m], want_out[m]);
        if (h_copied && h_copied[m] != want_k[m]) bad("copied", E::kBits, width, m, h_copied[m], want_k[m]);
        for (uint64_t s = src_start[m]; s < src_start[m + 1]; ++s)
            if (h_seg[s] != want_seg[s]) bad("segment crc", E::kBits, width, m, h_seg[s], want_seg[s]);
    }
    free(h_ss), free(h_ds), free(h_sl), free(h_dl), free(h_skip), free(h_size), free(h_seeds), free(h_seg), free(h_work),
        free(h_out), free(h_copied);
}

}  // namespace

int main() {
    uint32_t tab32[64];
    uint64_t tab64[64];
    power_table<Gf32>(xpow(8), tab32);
    power_table<Gf64>(xpow64(8), tab64);

    // window_bounds on its own, at the edges of 64 bits
    struct { uint64_t skip, size, L, D, a, k; } b[] = {
        {0, kAll, 600, 1000, 0, 600},  {150, kAll - 10, 600, 1000, 150, 450}, {kAll, kAll, 600, 1000, 600, 0},
        {600, 5, 600, 1000, 600, 0},   {599, 5, 600, 1000, 599, 1},           {10, 20, 600, 7, 10, 7},
        {10, 0, 600, 7, 10, 0},        {1, kAll, kAll, kAll, 1, kAll - 1},    {0, kAll, kAll, kAll, 0, kAll},
        {kAll - 1, 5, kAll, 9, kAll - 1, 1}, {5, 5, 0, 9, 0, 0},              {0, 5, 9, 0, 0, 0},
    };
    for (const auto& t : b) {
        const Window w = window_bounds(t.skip, t.size, t.L, t.D);
        if (w.a != t.a) bad("window_bounds a", 0, 0, (size_t)(&t - b), w.a, t.a);
        if (w.k != t.k) bad("window_bounds k", 0, 0, (size_t)(&t - b), w.k, t.k);
    }

    const std::vector<Case> all = cases();
    // the kernel's step width, and two that cut the source side elsewhere
    for (uint32_t width : {kUnscanStep, 1u, 7u})
        for (int mode = 0; mode < 3; ++mode) {
            run_call<E32>(all, mode, width, tab32);
            run_call<E64>(all, mode, width, tab64);
        }
    printf("window_finish_replay: %zu cases, %llu runs, %llu mismatches\n", all.size(), (unsigned long long)g_runs,
           (unsigned long long)g_bad);
    return g_bad ? 1 : 0;
}
