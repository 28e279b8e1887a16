// xor_kernels.h -- stripe parity + CRC in one read (photon_crc32c_xor_batch_*,
// photon_crc64ecma_xor_batch_*) and the expected parity CRC
// from stored block CRCs (photon_crc32c_xor_expect_n /
// photon_crc64ecma_xor_expect_n).
//
// Stripe s has k sources of n_s bytes and one parity range of n_s bytes. After
// the call the parity holds the byte-wise XOR P_s of the sources and
// out[s] = crc(P_s, seed_s). The kernels are the overwrite kernels' walk
// (overwrite_kernels.h: one group of G lanes per stripe, persistent grid,
// buf_geo's geometry, U rows per step) with k read streams and one write
// stream: the lane that owns a 16-byte block of a row loads that block from
// every source at the same offset, XORs the blocks into an accumulator, stores
// the accumulator and feeds it to the ONE CRC body. The geometry is taken on
// the parity; a source is addressed through its distance from the parity (a
// multiple of 16 on this route). They are kernels of their own beside the
// copying and the overwrite ones, so that no kernel that was here before
// changes; the table steps, finish, lane constants and table images are the
// shared ones.
//
// k is a run-time value. The sources are walked in chunks of kXorInFlight:
// the chunk's loads of all U rows are issued together, then folded into the
// accumulator. The first chunk's distances are kept in registers for the whole
// stripe and its loads for the NEXT step are issued before this step's CRC
// work, so a stripe of up to kXorInFlight sources has its loads in flight
// under the table lookups; later chunks take their pointers and their loads
// inside the step. A NULL source (the _ptr form) is an all-zero block: it is
// skipped, never loaded. The pointer is the same on every lane of a group.
//
// Ordering (the in-place accumulate: the parity range IS one source of its own
// stripe, same address and length). A byte of the parity is loaded and stored
// by lanes of ONE lane group, and a lane group never spans wavefronts. What a
// lane stores is the accumulator, taken through ow_after(): the store is
// issued behind the wait for all k loads of that block, the parity's own old
// block among them. Loads in flight at that point are later rows': other
// addresses. The head block's 16-byte loads cover up to 15 bytes in front of
// each range, which another lane group may be writing: they are masked on the
// accumulated XOR (all streams at once) and never reach the CRC or the store
// (store_head). Nothing behind a range's end is loaded in 16-byte blocks: the
// tail (< 16 bytes) goes byte by byte.
#pragma once
#include "overwrite_kernels.h"
#include "xor_expect.h"

// Sources whose loads are issued together per row (A/B builds: the Makefile's EXTRA).
#ifndef PCRC_XOR_INFLIGHT
#define PCRC_XOR_INFLIGHT 4
#endif

namespace pcrc {

constexpr int kXorInFlight = PCRC_XOR_INFLIGHT;
constexpr uint32_t kXorMaxSources = 64;

template <typename T>
struct XorArgs {
    const uint8_t* base;           // strided sources: base + s*stripe_stride + i*block_stride
    uint64_t stripe_stride;
    uint64_t block_stride;
    uint64_t nbytes;
    const void* const* src;        // _ptr form when non-null: count*k pointers, stripe-major; null = zeros
    const photon_crc_iovec* dstv;  // _ptr form: {parity, n_s}
    uint8_t* dst_base;             // strided parities
    uint64_t dst_stride;
    uint32_t k;
    uint64_t count;
    T seed0;
    const T* seeds;
    T* out;
};

// Source i of stripe s (null: an all-zero block).
template <typename T>
__device__ __forceinline__ const uint8_t* xor_src(const XorArgs<T>& a, uint64_t s, uint32_t i) {
    if (a.src) return static_cast<const uint8_t*>(a.src[s * a.k + i]);
    return a.base + s * a.stripe_stride + (uint64_t)i * a.block_stride;
}

// A chunk of kXorInFlight sources: where each lies relative to the parity.
struct XorChunk {
    ptrdiff_t dd[kXorInFlight];
    uint32_t on;  // bit j: source j of the chunk is there and not null
};

template <typename T>
__device__ __forceinline__ XorChunk xor_chunk(const XorArgs<T>& a, uint64_t s, uint32_t c, const uint8_t* dst) {
    XorChunk ch;
    ch.on = 0;
#pragma unroll
    for (int j = 0; j < kXorInFlight; ++j) {
        const uint32_t i = c * kXorInFlight + j;
        const uint8_t* p = i < a.k ? xor_src(a, s, i) : nullptr;
        ch.dd[j] = p ? p - dst : 0;
        if (p) ch.on |= 1u << j;
    }
    return ch;
}

__device__ __forceinline__ void xor_into(uint4& acc, const uint4& v) {
    acc.x ^= v.x;
    acc.y ^= v.y;
    acc.z ^= v.z;
    acc.w ^= v.w;
}

// The chunk's blocks at the parity addresses q[0..R): all loads issued
// together (act: this lane has blocks there).
template <int R>
__device__ __forceinline__ void xor_issue(const XorChunk& ch, const uint8_t* const* q, bool act,
                                          uint4 (&v)[R][kXorInFlight]) {
#pragma unroll
    for (int j = 0; j < kXorInFlight; ++j) {
        const bool on = act && ((ch.on >> j) & 1u);
#pragma unroll
        for (int r = 0; r < R; ++r) {
            v[r][j] = make_uint4(0, 0, 0, 0);
            if (on) v[r][j] = load16(q[r] + ch.dd[j]);
        }
    }
}

template <int R>
__device__ __forceinline__ void xor_fold(uint4 (&acc)[R], const uint4 (&v)[R][kXorInFlight]) {
#pragma unroll
    for (int j = 0; j < kXorInFlight; ++j)
#pragma unroll
        for (int r = 0; r < R; ++r) xor_into(acc[r], v[r][j]);
}

// The sources behind the first chunk, a chunk at a time, into acc.
template <int R, typename T>
__device__ __forceinline__ void xor_rest(const XorArgs<T>& a, uint64_t s, const uint8_t* dst,
                                         const uint8_t* const* q, bool act, uint4 (&acc)[R]) {
    for (uint32_t c = 1; c * kXorInFlight < a.k; ++c) {
        const XorChunk ch = xor_chunk(a, s, c, dst);
        uint4 v[R][kXorInFlight];
        xor_issue<R>(ch, q, act, v);
        xor_fold<R>(acc, v);
    }
}

// One block of every source XORed (a row outside the U-row steps).
template <typename T>
__device__ __forceinline__ uint4 xor_block(const XorArgs<T>& a, uint64_t s, const uint8_t* dst, const XorChunk& c0,
                                           const uint8_t* q, bool act) {
    const uint8_t* const qq[1] = {q};
    uint4 v[1][kXorInFlight];
    xor_issue<1>(c0, qq, act, v);
    uint4 acc[1] = {make_uint4(0, 0, 0, 0)};
    xor_fold<1>(acc, v);
    xor_rest<1>(a, s, dst, qq, act, acc);
    return acc[0];
}

// Byte `off` of the parity: the sources' bytes XORed, stored by the lane that
// owns it (mine); every lane that walks the bytes loads them.
template <typename T>
__device__ __forceinline__ uint8_t xor_byte(const XorArgs<T>& a, uint64_t s, uint8_t* dst, uint64_t off, bool mine) {
    uint32_t b = 0;
    for (uint32_t i = 0; i < a.k; ++i) {
        const uint8_t* p = xor_src(a, s, i);
        if (p) b ^= load8(p + off);
    }
    if (mine) store1(dst + off, (uint8_t)ow_after(b, b));
    return (uint8_t)b;
}

// What differs between the two CRCs in the walk below.
struct XorCrc32 {
    typedef uint32_t T;
    typedef uint32_t P;  // a lane's column partial
    typedef LaneAddr Addr;
    static constexpr bool kAllWalk = true;  // tiny stripes and tails: every lane of the group walks the bytes
    static __device__ __forceinline__ P lag(const uint32_t* lds, const uint4& w, const Addr& la) {
        return lag16(lds, w, la);
    }
    static __device__ __forceinline__ P step(const uint32_t* lds, P pc, const Addr& la, P c) {
        return sstep(lds, pc, la, c);
    }
    static __device__ __forceinline__ T byte(const uint32_t* lds, T r, uint8_t b, const Addr& la) {
        return bytestep(lds, r, b, la);
    }
    static __device__ __forceinline__ uint4 head(uint4 w, uint32_t gl, int s0, T init) {
        const int off = (int)gl * 16;
        w.x = head_word_sel(w.x, off, s0, init);
        w.y = head_word_sel(w.y, off + 4, s0, init);
        w.z = head_word_sel(w.z, off + 8, s0, init);
        w.w = head_word_sel(w.w, off + 12, s0, init);
        return w;
    }
    template <int G>
    static __device__ __forceinline__ T fin(const uint32_t* lds, P pc, uint32_t d, uint32_t, uint32_t,
                                            const Addr& la) {
        return finish_group<G>(lds, pc, d, la);
    }
};

struct XorCrc64 {
    typedef uint64_t T;
    typedef uint2 P;
    typedef LaneAddr64 Addr;
    static constexpr bool kAllWalk = false;  // the group's first lane alone, and the result is valid there
    static __device__ __forceinline__ P lag(const uint32_t* lds, const uint4& w, const Addr& la) {
        return lag16_64(lds, w, la);
    }
    static __device__ __forceinline__ P step(const uint32_t* lds, P pc, const Addr& la, P c) {
        return sstep64(lds, pc, la, c);
    }
    static __device__ __forceinline__ T byte(const uint32_t* lds, T r, uint8_t b, const Addr& la) {
        return bytestep64(lds, r, b, la);
    }
    static __device__ __forceinline__ uint4 head(uint4 w, uint32_t gl, int s0, T init) {
        if (gl < 2) {  // the head lies in the first two blocks
            const uint64_t lo = head_word64(((uint64_t)w.y << 32) | w.x, (int)gl * 16, s0, init);
            const uint64_t hi = head_word64(((uint64_t)w.w << 32) | w.z, (int)gl * 16 + 8, s0, init);
            w = make_uint4((uint32_t)lo, (uint32_t)(lo >> 32), (uint32_t)hi, (uint32_t)(hi >> 32));
        }
        return w;
    }
    template <int G>
    static __device__ __forceinline__ T fin(const uint32_t* lds, P pc, uint32_t d, uint32_t gl, uint32_t lane,
                                            const Addr&) {
        if constexpr (G == 16 && PCRC64_FIN16) {
            return finish_xor16(pc, d, lds, gl, lane);
        } else {
            const uint64_t f = finish64<G>(pc, d, lds, lane);
            return ((uint64_t)group_xor<G>((uint32_t)(f >> 32)) << 32) | group_xor<G>((uint32_t)f);
        }
    }
};

// The register after the parity of stripe s from `init` (CRC-32C: the seed
// and the CRC; CRC-64: ~seed and ~CRC) by a group of G lanes, the parity
// stored on the way. Every non-null source is co-aligned with dst, or n < 64.
// The loop is ow_reg32's without the second named stream: rows 1.. in steps
// of U, the rows left over one by one, the partial last row, the finish, the
// tail's bytes.
template <typename C, int G, int U>
__device__ __forceinline__ typename C::T xor_reg(const uint32_t* lds, const XorArgs<typename C::T>& a, uint64_t s,
                                                 uint8_t* dst, uint64_t n, typename C::T init, uint32_t gl,
                                                 uint32_t lane, const typename C::Addr& la) {
    typedef typename C::P P;
    typename C::T reg = init;
    const bool walk = C::kAllWalk || gl == 0;
    if (n < 64) {
        if (walk)
            for (uint64_t k = 0; k < n; ++k)
                reg = C::byte(lds, reg, xor_byte(a, s, dst, k, !C::kAllWalk || ((uint32_t)k & (G - 1)) == gl), la);
        return reg;
    }
    const BufGeo g = buf_geo<G>(dst, n, gl);
    uint8_t* lp = const_cast<uint8_t*>(g.lp);
    const XorChunk c0 = xor_chunk(a, s, 0, dst);
    // Row 0: the accumulated XOR stored from the data's first byte on; the
    // bytes in front of it masked (all streams at once) and the seed folded
    // in. The first step's loads of the first chunk are issued once row 0 is
    // accumulated, in front of its store and its lookups (issuing them with
    // row 0's own loads costs 16 more live VGPRs: the CRC-64 builds spill).
    const bool act0 = gl < g.nb;
    const bool step = 1 + U <= g.full;
    uint4 w0[1] = {xor_block(a, s, dst, c0, lp, act0)};
    uint4 v[U][kXorInFlight];
    const uint8_t* q[U];
#pragma unroll
    for (int u = 0; u < U; ++u) q[u] = lp + (1 + u) * (16 * G);
    xor_issue<U>(c0, q, step, v);
    if (act0) {
        const uint4 x = ow_after(w0[0], w0[0]);
        if (gl == 0 && g.s0) store_head(lp, x, g.s0);
        else store16(lp, x);
    }
    P pc = C::lag(lds, C::head(w0[0], gl, g.s0, init), la);
    uint64_t row = 1;
    if (step) {
        for (;;) {
            uint4 acc[U];
#pragma unroll
            for (int u = 0; u < U; ++u) acc[u] = make_uint4(0, 0, 0, 0);
            xor_fold<U>(acc, v);
            xor_rest<U>(a, s, dst, q, true, acc);
            uint8_t* at[U];
#pragma unroll
            for (int u = 0; u < U; ++u) at[u] = lp + (row + u) * (16 * G);
            row += U;
            const bool more = row + U <= g.full;
            // the next step's first chunk: in flight under this step's lookups
#pragma unroll
            for (int u = 0; u < U; ++u) q[u] = lp + (row + u) * (16 * G);
            xor_issue<U>(c0, q, more, v);
            P c[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                store16(at[u], ow_after(acc[u], acc[u]));
                c[u] = C::lag(lds, acc[u], la);
            }
#pragma unroll
            for (int u = 0; u < U; ++u) pc = C::step(lds, pc, la, c[u]);
            if (!more) break;
        }
    }
    for (; row < g.full; ++row) {
        uint8_t* at = lp + row * (16 * G);
        const uint4 x = xor_block(a, s, dst, c0, at, true);
        store16(at, ow_after(x, x));
        pc = C::step(lds, pc, la, C::lag(lds, x, la));
    }
    if (g.full >= 1 && g.full < g.rows && g.full * G + gl < g.nb) {  // the partial last row
        uint8_t* at = lp + g.full * (16 * G);
        const uint4 x = xor_block(a, s, dst, c0, at, true);
        store16(at, ow_after(x, x));
        pc = C::step(lds, pc, la, C::lag(lds, x, la));
    }
    const uint32_t d = (g.rlast + G - 1 - gl) & (G - 1);
    reg = C::template fin<G>(lds, pc, d, gl, lane, la);
    if (walk)
        for (const uint8_t* t = g.eb; t < g.e; ++t)
            reg = C::byte(lds, reg,
                          xor_byte(a, s, dst, (uint64_t)(t - dst), !C::kAllWalk || ((uint32_t)(t - g.eb) & (G - 1)) == gl),
                          la);
    return reg;
}

// Stripe s of the wave's lane group: parity and length (nothing for a group
// behind the batch's end).
template <typename T>
__device__ __forceinline__ void xor_item(const XorArgs<T>& a, uint64_t s, uint8_t** d, uint64_t* n) {
    *d = nullptr;
    *n = 0;
    if (s < a.count) {
        if (a.dstv) {
            *d = static_cast<uint8_t*>(const_cast<void*>(a.dstv[s].base));
            *n = a.dstv[s].len;
        } else {
            *d = a.dst_base + s * a.dst_stride;
            *n = a.nbytes;
        }
    }
}

// True when every non-null source of stripe s is congruent to dst modulo 16.
template <typename T>
__device__ __forceinline__ bool xor_coaligned(const XorArgs<T>& a, uint64_t s, const uint8_t* dst) {
    uint32_t mis = 0;
    for (uint32_t i = 0; i < a.k; ++i) {
        const uint8_t* p = xor_src(a, s, i);
        if (p) mis |= (uint32_t)(p - dst) & 15u;
    }
    return mis == 0;
}

// A stripe that is NOT co-aligned (n >= 64; correctness only, as the copying
// kernels' group_copy): the parity landed byte by byte, byte b by lane b mod
// G, which loads that byte of every source first (in place: the parity's own
// old byte among them, loaded and stored by the same lane). The CRC is then
// taken over the parity itself, behind a fence: every lane of the
// group reads bytes that other lanes of its wavefront stored.
template <int G, typename T>
__device__ __forceinline__ void xor_land_bytes(const XorArgs<T>& a, uint64_t s, uint8_t* dst, uint64_t n, uint32_t gl) {
    for (uint64_t b = gl; b < n; b += G) xor_byte(a, s, dst, b, true);
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
}

template <int G, int U>
__global__ __launch_bounds__(kBlock) void crc32c_xor_kernel(XorArgs<uint32_t> a, LaneConsts kc) {
    __shared__ __attribute__((aligned(16))) uint32_t lds[lds_bytes_for<G>() / 4];
    load_tables<G>(lds, kc);
    constexpr int GPW = 64 / G;
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t gl = lane & (G - 1);
    const uint32_t grp = lane / G;
    const LaneAddr la = lane_addr(lane);
    const uint64_t nwaves = (uint64_t)gridDim.x * kWaves;
    for (uint64_t wv = (uint64_t)blockIdx.x * kWaves + wave_id(); wv * GPW < a.count; wv += nwaves) {
        const uint64_t s = wv * GPW + grp;
        uint8_t* dst;
        uint64_t n;
        xor_item(a, s, &dst, &n);
        uint32_t seed = a.seed0;
        if (s < a.count && a.seeds) seed = a.seeds[s];
        uint32_t crc;
        if (n < 64 || xor_coaligned(a, s, dst)) {
            crc = xor_reg<XorCrc32, G, U>(lds, a, s, dst, n, seed, gl, lane, la);
        } else {
            xor_land_bytes<G>(a, s, dst, n, gl);
            crc = buffer_crc<G, U>(lds, dst, n, seed, gl, la);
        }
        if (s < a.count && gl == 0) a.out[s] = crc;
    }
}

template <int G, int U>
__global__ __launch_bounds__(kBlock) void crc64_xor_kernel(XorArgs<uint64_t> a, LaneConsts64 kc) {
    __shared__ __attribute__((aligned(16))) uint32_t lds[k64FLdsBytes / 4];
    load_tables64<G>(lds, kc);
    constexpr int GPW = 64 / G;
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t gl = lane & (G - 1);
    const uint32_t grp = lane / G;
    const LaneAddr64 la = lane_addr64(lane);
    const uint64_t nwaves = (uint64_t)gridDim.x * kWaves;
    for (uint64_t wv = (uint64_t)blockIdx.x * kWaves + wave_id(); wv * GPW < a.count; wv += nwaves) {
        const uint64_t s = wv * GPW + grp;
        uint8_t* dst;
        uint64_t n;
        xor_item(a, s, &dst, &n);
        uint64_t seed = a.seed0;
        if (s < a.count && a.seeds) seed = a.seeds[s];
        // crc.cpp:119-122: the register starts at ~crc and the result is inverted
        uint64_t reg;
        if (n < 64 || xor_coaligned(a, s, dst)) {
            reg = xor_reg<XorCrc64, G, U>(lds, a, s, dst, n, ~seed, gl, lane, la);
        } else {
            xor_land_bytes<G>(a, s, dst, n, gl);
            reg = buffer_reg64<G, false, 4>(lds, dst, n, ~seed, gl, lane, la);
        }
        if (s < a.count && gl == 0) a.out[s] = ~reg;
    }
}

// photon_crc32c_xor_expect_n / photon_crc64ecma_xor_expect_n: a thread per
// stripe (groups are a stripe's blocks: small), xor_expect_stripe. Plain loads
// and stores only; nothing but want[s] is written.
constexpr int kXorExpectBlock = 256;
template <typename G, typename P>
__global__ __launch_bounds__(kXorExpectBlock) void xor_expect_kernel(const typename G::T* crc, uint64_t ncrc,
                                                                     const uint64_t* grp_start, uint32_t k,
                                                                     const uint64_t* len, uint64_t nbytes,
                                                                     uint64_t count, typename G::T seed,
                                                                     typename G::T inv, typename G::T* want, P pt) {
    for (uint64_t s = (uint64_t)blockIdx.x * kXorExpectBlock + threadIdx.x; s < count;
         s += (uint64_t)gridDim.x * kXorExpectBlock)
        want[s] = xor_expect_stripe<G>(crc, ncrc, grp_start, k, len, nbytes, s, seed, inv, pt.x8pow2);
}

}  // namespace pcrc
