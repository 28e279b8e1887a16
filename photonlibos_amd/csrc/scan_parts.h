// scan_parts.h -- the running CRCs of an object's parts
// (photon_crc32c_scan_parts_n / photon_crc64ecma_scan_parts_n, DESIGN.md
// §4.11), written once for the device kernels (scan_reduce_kernel,
// scan_carry_kernel, scan_apply_kernel in crc32c_kernels.h) and for the CPU
// replay of them (photon_crc_test_scan_parts, tuning.h).
//
// Over an object's parts s in order, from A = seed_m, E = 0:
//   A = A * x^(8 len[s]) ^ crc[s], run[s] = A;   E += len[s], end[s] = E
// (the fold's definition, fold_parts.h, with every intermediate value kept).
// It is a segmented scan over the index space [0, nparts) under the monoid of
// the element (v, f, bytes, closed): the map state -> state of a stretch of
// entries, state = (A, E). An open stretch maps (A, E) to (A * f ^ v,
// E + bytes), f = the product of its x^(8 len); a closed one holds the start
// of an object and maps every state to (v, bytes). Entry 0 always starts an
// object, so every prefix is closed and a carry is a state.
//
//   reduce  a workgroup per tile of `tile` entries (a power of two, 64 ...
//           65,536), whatever objects it holds: thread t reduces its run of
//           consecutive entries (scan_run), the runs combine in thread order
//           (scan_combine), the tile's element goes to the workspace.
//   carry   one workgroup: the tiles' elements become their exclusive
//           prefixes, in place, in chunks of kScanChunk tiles with the carry
//           handed from chunk to chunk.
//   apply   a workgroup per tile: thread t's Horner chain (scan_emit) from
//           the tile's carry combined with the runs before t's.
// One tile needs apply alone.
//
// Workspace: 4 * tiles words of 64 bits: [0, tiles) v, [tiles, 2 tiles) f,
// [2 tiles, 3 tiles) bytes, [3 tiles, 4 tiles) closed. Every word a call reads
// it has written before: the workspace needs no clearing and keeps nothing.
#pragma once
#include <stdint.h>

#include "fold_parts.h"

// as PCRC_HD, for the steps that walk arrays (not constant expressions)
#ifndef PCRC_VHD
#ifdef __HIPCC__
#define PCRC_VHD __host__ __device__ inline
#else
#define PCRC_VHD inline
#endif
#endif

namespace pcrc {

constexpr uint32_t kScanMinTile = 64, kScanMaxTile = 65536;
#ifndef PCRC_SCAN_BLOCK  // A/B builds (the Makefile's EXTRA): a power of two, 64 ... 1024
#define PCRC_SCAN_BLOCK 256
#endif
constexpr uint32_t kScanBlock = PCRC_SCAN_BLOCK;  // threads of a reduce / apply workgroup (fewer for smaller tiles)
constexpr uint32_t kScanChunk = 256;    // threads of the carry workgroup = tiles per chunk
constexpr uint32_t kScanMaxGrid = 2048; // workgroups of reduce / apply; tiles beyond: a stride loop
constexpr uint64_t kScanMaxParts = 1ull << 40;  // parts of one call
constexpr uint64_t kScanNone = ~0ull;

PCRC_HD bool scan_tile_ok(uint64_t tile) {
    return tile >= kScanMinTile && tile <= kScanMaxTile && !(tile & (tile - 1));
}
PCRC_HD uint64_t scan_tiles(uint64_t nparts, uint32_t tile) { return (nparts + tile - 1) / tile; }
// ~0: more parts than one call takes
PCRC_HD uint64_t scan_work_words(uint64_t nparts, uint32_t tile) {
    return nparts > kScanMaxParts ? kScanNone : 4 * scan_tiles(nparts, tile);
}
PCRC_HD uint32_t scan_block(uint32_t tile) { return tile < kScanBlock ? tile : kScanBlock; }

// Threads of nt with a run over n entries (fold_run_bounds: the first ones).
PCRC_HD uint32_t scan_active(uint64_t n, uint32_t nt) {
    const uint64_t per = (n + nt - 1) / nt;
    return per ? (uint32_t)((n + per - 1) / per) : 0u;
}

template <typename T>
struct ScanElem {
    T v, f;           // state (A, E) -> (A * f ^ v, E + bytes); closed: -> (v, bytes), f unused
    uint64_t bytes;
    uint32_t closed;
};

template <typename G>
PCRC_HD ScanElem<typename G::T> scan_identity() {
    return ScanElem<typename G::T>{0, G::one(), 0, 0};
}

// a, then b.
template <typename G>
PCRC_HD ScanElem<typename G::T> scan_combine(const ScanElem<typename G::T>& a, const ScanElem<typename G::T>& b) {
    if (b.closed) return b;
    ScanElem<typename G::T> r = a;
    r.v = (a.v ? G::mul(a.v, b.f) : 0) ^ b.v;
    if (!a.closed) r.f = G::mul(a.f, b.f);
    r.bytes = a.bytes + b.bytes;
    return r;
}

template <typename T>
PCRC_VHD void scan_store(uint64_t* work, uint64_t tiles, uint64_t k, const ScanElem<T>& e) {
    work[k] = e.v;
    work[tiles + k] = e.f;
    work[2 * tiles + k] = e.bytes;
    work[3 * tiles + k] = e.closed;
}
template <typename T>
PCRC_VHD ScanElem<T> scan_load(const uint64_t* work, uint64_t tiles, uint64_t k) {
    return ScanElem<T>{(T)work[k], (T)work[tiles + k], work[2 * tiles + k], (uint32_t)work[3 * tiles + k]};
}

// Where a walk over the entries stands among the objects: m = the last object
// that starts at or before the entry at hand, next = where object m + 1 starts
// (~0 behind the last object), fresh = the entry the cursor was made at starts
// an object. Only obj_start[0 .. nobj) is ever read, and m stays below nobj:
// an obj_start that breaks its rules gives other values, never another access.
struct ScanCursor {
    uint64_t m, next;
    bool fresh;
};

PCRC_VHD uint64_t scan_next_start(const uint64_t* obj_start, uint64_t nobj, uint64_t m) {
    return obj_start && m + 1 < nobj ? obj_start[m + 1] : kScanNone;
}

// The cursor at entry s, by binary search (a null obj_start: one object).
PCRC_VHD ScanCursor scan_cursor(const uint64_t* obj_start, uint64_t nobj, uint64_t s) {
    uint64_t a = 0, b = obj_start ? nobj : 1;  // the object is in [a, b)
    while (b - a > 1) {
        const uint64_t mid = a + (b - a) / 2;
        if (obj_start[mid] <= s) a = mid;
        else b = mid;
    }
    return ScanCursor{a, scan_next_start(obj_start, nobj, a), s == 0 || (obj_start && obj_start[a] == s)};
}

// Does entry s start an object? (entries in ascending order from the cursor's)
// Objects that start at s and are empty are passed over: m ends at the last.
PCRC_VHD bool scan_starts(ScanCursor* c, const uint64_t* obj_start, uint64_t nobj, uint64_t s) {
    bool st = c->fresh;
    c->fresh = false;
    while (s >= c->next) {
        ++c->m;
        c->next = scan_next_start(obj_start, nobj, c->m);
        st = true;
    }
    return st;
}

// The inputs of a call, as the kernels get them.
template <typename T>
struct ScanIn {
    const T* crc;
    const uint64_t* len;
    const uint64_t* obj_start;
    uint64_t nobj, nparts;
    T seed0;
    const T* seeds;
};

// The reduce step of one thread: the element of entries [lo, hi). The
// multiplier x^(8 len) is kept while consecutive lengths repeat (as fold_run).
template <typename G>
PCRC_VHD ScanElem<typename G::T> scan_run(const ScanIn<typename G::T>& in, uint64_t lo, uint64_t hi,
                                          const typename G::T* tab) {
    typedef typename G::T T;
    ScanElem<T> e = scan_identity<G>();
    if (lo >= hi) return e;
    ScanCursor c = scan_cursor(in.obj_start, in.nobj, lo);
    uint64_t klen = 0;
    T k = G::one();  // x^(8 * klen)
    for (uint64_t s = lo; s < hi; ++s) {
        const uint64_t n = in.len[s];
        const T x = in.crc[s];
        if (n != klen) {
            k = fold_xpow8<G>(n, tab);
            klen = n;
        }
        if (scan_starts(&c, in.obj_start, in.nobj, s)) {
            e.v = in.seeds ? in.seeds[c.m] : in.seed0;
            e.bytes = 0;
            e.closed = 1;
        } else if (!e.closed) {
            e.f = G::mul(e.f, k);
        }
        e.v = (e.v ? G::mul(e.v, k) : 0) ^ x;
        e.bytes += n;
    }
    return e;
}

// The apply step of one thread: the chain over entries [lo, hi) from the
// state `before` = everything in front of lo, each value stored.
template <typename G>
PCRC_VHD void scan_emit(const ScanIn<typename G::T>& in, uint64_t lo, uint64_t hi, const typename G::T* tab,
                        const ScanElem<typename G::T>& before, typename G::T* run, uint64_t* end) {
    typedef typename G::T T;
    if (lo >= hi) return;
    ScanCursor c = scan_cursor(in.obj_start, in.nobj, lo);
    T acc = before.v;
    uint64_t bytes = before.bytes, klen = 0;
    T k = G::one();
    for (uint64_t s = lo; s < hi; ++s) {
        const uint64_t n = in.len[s];
        const T x = in.crc[s];
        if (n != klen) {
            k = fold_xpow8<G>(n, tab);
            klen = n;
        }
        if (scan_starts(&c, in.obj_start, in.nobj, s)) {
            acc = in.seeds ? in.seeds[c.m] : in.seed0;
            bytes = 0;
        }
        acc = (acc ? G::mul(acc, k) : 0) ^ x;
        bytes += n;
        run[s] = acc;
        if (end) end[s] = bytes;
    }
}

PCRC_HD uint64_t scan_tile_end(uint64_t nparts, uint32_t tile, uint64_t k) {
    return nparts - k * tile < tile ? nparts : k * tile + tile;
}

// The three steps in order over host arrays, for workgroups of nt threads
// (the CPU replay of the kernels; the kernels combine a tile's runs and a
// chunk's tiles by a scan through LDS). work: scan_work_words(nparts, tile)
// words, uninitialised.
template <typename G>
inline void scan_replay(const ScanIn<typename G::T>& in, uint32_t tile, uint32_t nt, const typename G::T* tab,
                        uint64_t* work, typename G::T* run, uint64_t* end) {
    typedef typename G::T T;
    const uint64_t tiles = scan_tiles(in.nparts, tile);
    if (tiles > 1) {
        for (uint64_t k = 0; k < tiles; ++k) {  // reduce
            const uint64_t lo = k * tile, hi = scan_tile_end(in.nparts, tile, k);
            ScanElem<T> all = scan_identity<G>();
            for (uint32_t t = 0; t < nt; ++t) {
                uint64_t a, b;
                fold_run_bounds(hi - lo, nt, t, &a, &b);
                all = scan_combine<G>(all, scan_run<G>(in, lo + a, lo + b, tab));
            }
            scan_store<T>(work, tiles, k, all);
        }
        ScanElem<T> carry = scan_identity<G>();  // carry
        for (uint64_t c0 = 0; c0 < tiles; c0 += kScanChunk)
            for (uint64_t k = c0; k < tiles && k < c0 + kScanChunk; ++k) {
                const ScanElem<T> e = scan_load<T>(work, tiles, k);
                scan_store<T>(work, tiles, k, carry);
                carry = scan_combine<G>(carry, e);
            }
    }
    for (uint64_t k = 0; k < tiles; ++k) {  // apply
        const uint64_t lo = k * tile, hi = scan_tile_end(in.nparts, tile, k);
        ScanElem<T> before = tiles > 1 ? scan_load<T>(work, tiles, k) : scan_identity<G>();
        for (uint32_t t = 0; t < nt; ++t) {
            uint64_t a, b;
            fold_run_bounds(hi - lo, nt, t, &a, &b);
            scan_emit<G>(in, lo + a, lo + b, tab, before, run, end);
            before = scan_combine<G>(before, scan_run<G>(in, lo + a, lo + b, tab));
        }
    }
}

}  // namespace pcrc
