// overwrite_kernels.h -- overwrite + CRC delta (photon_crc32c_overwrite_batch_*,
// photon_crc64ecma_overwrite_batch_*) and the patch of stored
// CRCs by the deltas (photon_crc32c_patch_n / photon_crc64ecma_patch_n).
//
// Write i replaces the n_i bytes O at dst_i by the source bytes N, and
// delta[i] = R(O xor N), the raw CRC from a zero register: the XOR of the old
// and the new CRC of the range from any common seed. The kernels are the
// copying batch kernels' walk (crc32c_batch_kernel<G, U, 0, true>,
// crc64_batch_kernel<G, true>: one group of G lanes per buffer, persistent
// grid, U rows per step with the next U in flight) with a second stream: the
// lane that loads a 16-byte source block also loads the old block at the same
// offset from the destination's aligned start, feeds `src xor old` to the CRC
// and stores the raw source block. They are kernels of their own beside the
// copying ones, with row loops of their own (ow_reg32 / ow_reg64), so that no
// kernel that was here before changes; the table steps, finish, lane
// constants and table images are the shared ones.
//
// Ordering. A byte of the destination is loaded and stored by lanes of ONE
// lane group, and a lane group never spans wavefronts. Every store takes its
// data through ow_after(), an empty asm statement that makes the stored
// registers depend on the XOR of the two loaded blocks: the store instruction
// is therefore issued behind the s_waitcnt on both loads, the old block's
// among them. Rows in flight are loads of LATER rows: other addresses.
// A head block's 16-byte old load covers up to 15 bytes in front of the
// destination, which another lane group may be overwriting: they are masked
// exactly as the source's (head_word_sel / head_word64 with a zero seed), and
// whatever they held never reaches the CRC. Nothing behind the destination's
// end is loaded in 16-byte blocks: the tail (< 16 bytes) goes byte by byte.
#pragma once
#include "crc64_kernels.h"
#include "patch_crc.h"

// Bench-only ablation builds of the overwrite kernels (-DPCRC_OW_ABL=bits,
// DESIGN.md §4.14; 0 in the product): 1 = stores not made to depend on the old
// load (ow_after hands its value back untouched), 2 = old blocks by streaming
// loads (load16) instead of plain ones.
#ifndef PCRC_OW_ABL
#define PCRC_OW_ABL 0
#endif

namespace pcrc {

template <typename T>
struct OverwriteArgs {
    const uint8_t* base;          // strided sources
    uint64_t stride;
    uint64_t nbytes;
    const photon_crc_iovec* iov;  // iov mode when non-null
    uint64_t count;
    uint8_t* dst_base;            // strided destinations (dst null)
    uint64_t dst_stride;
    void* const* dst;
    T* out;                       // the deltas
};

// v as it is, made to depend on x (no instruction): what is stored from v is
// stored behind the wait for everything x was computed from.
__device__ __forceinline__ uint4 ow_after(uint4 v, const uint4& x) {
    if constexpr ((PCRC_OW_ABL & 1) != 0) return v;
    asm volatile("" : "+v"(v.x), "+v"(v.y), "+v"(v.z), "+v"(v.w) : "v"(x.x), "v"(x.y), "v"(x.z), "v"(x.w));
    return v;
}
__device__ __forceinline__ uint32_t ow_after(uint32_t v, uint32_t x) {
    if constexpr ((PCRC_OW_ABL & 1) != 0) return v;
    asm volatile("" : "+v"(v) : "v"(x));
    return v;
}

// The old block: a plain 16-byte load, not load16's streaming one -- the same
// lane stores over the line next (measured: 2 to 3.5 % of the launch on the
// full shapes).
__device__ __forceinline__ uint4 ow_load_old(const uint8_t* p) {
    if constexpr ((PCRC_OW_ABL & 2) != 0) return load16(p);
    const u32x4 v = *(g_u32x4*)p;
    return make_uint4(v.x, v.y, v.z, v.w);
}

// A 16-byte source block and the old block it replaces (OW; else zero: the
// plain CRC of one stream, for the buffers that are not co-aligned).
struct OwBlk {
    uint4 s, o;
};
template <bool OW>
__device__ __forceinline__ OwBlk ow_load(const uint8_t* q, ptrdiff_t dd) {
    OwBlk b;
    b.s = load16(q);
    if constexpr (OW) b.o = ow_load_old(q + dd);
    else b.o = make_uint4(0, 0, 0, 0);
    return b;
}
__device__ __forceinline__ uint4 ow_xor(const OwBlk& b) {
    return make_uint4(b.s.x ^ b.o.x, b.s.y ^ b.o.y, b.s.z ^ b.o.z, b.s.w ^ b.o.w);
}
// The block the CRC takes; OW: the source block stored over the old one.
template <bool OW>
__device__ __forceinline__ uint4 ow_take(const OwBlk& b, const uint8_t* q, ptrdiff_t dd) {
    const uint4 x = ow_xor(b);
    if constexpr (OW) store16(const_cast<uint8_t*>(q) + dd, ow_after(b.s, x));
    return x;
}
// Byte k of a tiny buffer or a tail; stored by lane k mod G of the group
// (mine), every lane of the group loads it.
template <bool OW>
__device__ __forceinline__ uint8_t ow_byte(const uint8_t* q, ptrdiff_t dd, bool mine) {
    const uint8_t b = load8(q);
    if constexpr (OW) {
        const uint8_t x = b ^ load8(q + dd);
        if (mine) store1(const_cast<uint8_t*>(q) + dd, (uint8_t)ow_after((uint32_t)b, (uint32_t)x));
        return x;
    }
    return b;
}

// R(src xor old) of one buffer by a group of G lanes (OW; dd = destination -
// source, a multiple of 16 unless n < 64), or R(src) alone and no store
// (!OW). Valid on every lane of the group. The geometry is buf_geo's, the
// loop buf_body's rolling reload without lead rows, the finish buf_finish's.
template <int G, int U, bool OW>
__device__ __forceinline__ uint32_t ow_reg32(const uint32_t* lds, const uint8_t* p, uint64_t n, ptrdiff_t dd,
                                             uint32_t gl, const LaneAddr& la) {
    uint32_t crc = 0;
    if (n < 64) {
        for (uint64_t k = 0; k < n; ++k)
            crc = bytestep(lds, crc, ow_byte<OW>(p + k, dd, ((uint32_t)k & (G - 1)) == gl), la);
        return crc;
    }
    const BufGeo g = buf_geo<G>(p, n, gl);
    // Row 0 and the first step's rows together; a lane without a block there
    // re-reads the aligned start (in bounds on both streams; discarded).
    const uint8_t* p0 = gl < g.nb ? g.lp : g.a0;
    const OwBlk b0 = ow_load<OW>(p0, dd);
    const bool step = 1 + U <= g.full;
    OwBlk cur[U];
#pragma unroll
    for (int u = 0; u < U; ++u) cur[u] = ow_load<OW>(step ? g.lp + (1 + u) * (16 * G) : p0, dd);
    // Row 0: the bytes in front of the data masked on the XOR (both streams
    // at once); the raw source block stored from the data's first byte on.
    uint4 w = ow_xor(b0);
    if constexpr (OW) {
        if (gl < g.nb) {
            uint8_t* d = const_cast<uint8_t*>(g.lp) + dd;
            const uint4 s = ow_after(b0.s, w);
            if (gl == 0 && g.s0) store_head(d, s, g.s0);
            else store16(d, s);
        }
    }
    const int off = (int)gl * 16;
    w.x = head_word_sel(w.x, off, g.s0, 0u);
    w.y = head_word_sel(w.y, off + 4, g.s0, 0u);
    w.z = head_word_sel(w.z, off + 8, g.s0, 0u);
    w.w = head_word_sel(w.w, off + 12, g.s0, 0u);
    if (gl >= g.nb) w = make_uint4(0, 0, 0, 0);
    uint32_t pc = lag16(lds, w, la);
    uint64_t row = 1;
    const uint8_t* lp = g.lp;
    if (step) {
        for (; row + 2 * U <= g.full; row += U) {
            uint32_t c[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                c[u] = lag16(lds, ow_take<OW>(cur[u], lp + (row + u) * (16 * G), dd), la);
                cur[u] = ow_load<OW>(lp + (row + U + u) * (16 * G), dd);
            }
#pragma unroll
            for (int u = 0; u < U; ++u) pc = sstep(lds, pc, la, c[u]);
        }
        uint32_t c[U];
#pragma unroll
        for (int u = 0; u < U; ++u) c[u] = lag16(lds, ow_take<OW>(cur[u], lp + (row + u) * (16 * G), dd), la);
#pragma unroll
        for (int u = 0; u < U; ++u) pc = sstep(lds, pc, la, c[u]);
        row += U;
    }
    for (; row < g.full; ++row) {
        const uint8_t* q = lp + row * (16 * G);
        pc = sstep(lds, pc, la, lag16(lds, ow_take<OW>(ow_load<OW>(q, dd), q, dd), la));
    }
    if (g.full >= 1 && g.full < g.rows && g.full * G + gl < g.nb) {  // the partial last row
        const uint8_t* q = lp + g.full * (16 * G);
        pc = sstep(lds, pc, la, lag16(lds, ow_take<OW>(ow_load<OW>(q, dd), q, dd), la));
    }
    const uint32_t d = (g.rlast + G - 1 - gl) & (G - 1);
    crc = finish_group<G>(lds, pc, d, la);
    for (const uint8_t* q = g.eb; q < g.e; ++q)
        crc = bytestep(lds, crc, ow_byte<OW>(q, dd, ((uint32_t)(q - g.eb) & (G - 1)) == gl), la);
    return crc;
}

// The same for CRC-64/ECMA: the raw register from 0 (the inversions of
// crc64ecma_extend cancel in the XOR of two CRCs). As buffer_reg64, the tiny
// buffer's and the tail's bytes are walked by the group's first lane alone,
// and the result is valid there.
template <int G, int U, bool OW>
__device__ __forceinline__ uint64_t ow_reg64(const uint32_t* lds, const uint8_t* p, uint64_t n, ptrdiff_t dd,
                                             uint32_t gl, uint32_t lane, const LaneAddr64& la) {
    uint64_t reg = 0;
    if (n < 64) {
        if (gl == 0)
            for (uint64_t k = 0; k < n; ++k) reg = bytestep64(lds, reg, ow_byte<OW>(p + k, dd, true), la);
        return reg;
    }
    const BufGeo g = buf_geo<G>(p, n, gl);
    const uint8_t* p0 = gl < g.nb ? g.lp : g.a0;
    const OwBlk b0 = ow_load<OW>(p0, dd);
    const bool step = 1 + U <= g.full;
    OwBlk cur[U];
#pragma unroll
    for (int u = 0; u < U; ++u) cur[u] = ow_load<OW>(step ? g.lp + (1 + u) * (16 * G) : p0, dd);
    uint4 w = ow_xor(b0);
    if constexpr (OW) {
        if (gl < g.nb) {
            uint8_t* d = const_cast<uint8_t*>(g.lp) + dd;
            const uint4 s = ow_after(b0.s, w);
            if (gl == 0 && g.s0) store_head(d, s, g.s0);
            else store16(d, s);
        }
    }
    if (gl < 2) {  // the head lies in the first two blocks
        const uint64_t lo = head_word64(((uint64_t)w.y << 32) | w.x, (int)gl * 16, g.s0, 0ull);
        const uint64_t hi = head_word64(((uint64_t)w.w << 32) | w.z, (int)gl * 16 + 8, g.s0, 0ull);
        w = make_uint4((uint32_t)lo, (uint32_t)(lo >> 32), (uint32_t)hi, (uint32_t)(hi >> 32));
    }
    if (gl >= g.nb) w = make_uint4(0, 0, 0, 0);
    uint2 pc = lag16_64(lds, w, la);
    uint64_t row = 1;
    const uint8_t* lp = g.lp;
    if (step) {
        for (; row + 2 * U <= g.full; row += U) {
            uint2 c[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                c[u] = lag16_64(lds, ow_take<OW>(cur[u], lp + (row + u) * (16 * G), dd), la);
                cur[u] = ow_load<OW>(lp + (row + U + u) * (16 * G), dd);
            }
#pragma unroll
            for (int u = 0; u < U; ++u) pc = sstep64(lds, pc, la, c[u]);
        }
        uint2 c[U];
#pragma unroll
        for (int u = 0; u < U; ++u) c[u] = lag16_64(lds, ow_take<OW>(cur[u], lp + (row + u) * (16 * G), dd), la);
#pragma unroll
        for (int u = 0; u < U; ++u) pc = sstep64(lds, pc, la, c[u]);
        row += U;
    }
    for (; row < g.full; ++row) {
        const uint8_t* q = lp + row * (16 * G);
        pc = sstep64(lds, pc, la, lag16_64(lds, ow_take<OW>(ow_load<OW>(q, dd), q, dd), la));
    }
    if (g.full >= 1 && g.full < g.rows && g.full * G + gl < g.nb) {
        const uint8_t* q = lp + g.full * (16 * G);
        pc = sstep64(lds, pc, la, lag16_64(lds, ow_take<OW>(ow_load<OW>(q, dd), q, dd), la));
    }
    const uint32_t d = (g.rlast + G - 1 - gl) & (G - 1);
    if constexpr (G == 16 && PCRC64_FIN16) {
        reg = finish_xor16(pc, d, lds, gl, lane);
    } else {
        const uint64_t f = finish64<G>(pc, d, lds, lane);
        reg = ((uint64_t)group_xor<G>((uint32_t)(f >> 32)) << 32) | group_xor<G>((uint32_t)f);
    }
    if (gl == 0)
        for (const uint8_t* q = g.eb; q < g.e; ++q) reg = bytestep64(lds, reg, ow_byte<OW>(q, dd, true), la);
    return reg;
}

// Write bi of the wave's lane group: source, length, destination (nothing
// for a group behind the batch's end).
template <typename T>
__device__ __forceinline__ void ow_item(const OverwriteArgs<T>& a, uint64_t bi, const uint8_t** p, uint64_t* n,
                                        uint8_t** d) {
    *p = nullptr;
    *n = 0;
    *d = nullptr;
    if (bi < a.count) {
        if (a.iov) {
            *p = static_cast<const uint8_t*>(a.iov[bi].base);
            *n = a.iov[bi].len;
        } else {
            *p = a.base + bi * a.stride;
            *n = a.nbytes;
        }
        *d = a.dst ? static_cast<uint8_t*>(a.dst[bi]) : a.dst_base + bi * a.dst_stride;
    }
}

// A buffer whose destination is NOT co-aligned with its source (n >= 64;
// correctness only, as the copying kernels' group_copy): R(old) and R(src)
// one after the other with stores off, then group_copy, whose lane index is
// made to depend on the delta (ow_after) -- on every old byte the group
// loaded -- so that its stores are issued behind all of those loads.
template <int G, int U>
__global__ __launch_bounds__(kBlock) void crc32c_overwrite_kernel(OverwriteArgs<uint32_t> a, LaneConsts kc) {
    __shared__ __attribute__((aligned(16))) uint32_t lds[lds_bytes_for<G>() / 4];
    load_tables<G>(lds, kc);
    constexpr int GPW = 64 / G;
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t gl = lane & (G - 1);
    const uint32_t grp = lane / G;
    const LaneAddr la = lane_addr(lane);
    const uint64_t nwaves = (uint64_t)gridDim.x * kWaves;
    for (uint64_t wv = (uint64_t)blockIdx.x * kWaves + wave_id(); wv * GPW < a.count; wv += nwaves) {
        const uint64_t bi = wv * GPW + grp;
        const uint8_t* p;
        uint64_t n;
        uint8_t* dst;
        ow_item(a, bi, &p, &n, &dst);
        const ptrdiff_t dd = dst - p;
        uint32_t delta;
        if (n < 64 || (dd & 15) == 0) {
            delta = ow_reg32<G, U, true>(lds, p, n, dd, gl, la);
        } else {
            delta = ow_reg32<G, 1, false>(lds, dst, n, 0, gl, la);
            delta ^= ow_reg32<G, 1, false>(lds, p, n, 0, gl, la);
            group_copy<G>(p, dst, n, ow_after(gl, delta));
        }
        if (bi < a.count && gl == 0) a.out[bi] = delta;
    }
}

template <int G, int U>
__global__ __launch_bounds__(kBlock) void crc64_overwrite_kernel(OverwriteArgs<uint64_t> a, LaneConsts64 kc) {
    __shared__ __attribute__((aligned(16))) uint32_t lds[k64FLdsBytes / 4];
    load_tables64<G>(lds, kc);
    constexpr int GPW = 64 / G;
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t gl = lane & (G - 1);
    const uint32_t grp = lane / G;
    const LaneAddr64 la = lane_addr64(lane);
    const uint64_t nwaves = (uint64_t)gridDim.x * kWaves;
    for (uint64_t wv = (uint64_t)blockIdx.x * kWaves + wave_id(); wv * GPW < a.count; wv += nwaves) {
        const uint64_t bi = wv * GPW + grp;
        const uint8_t* p;
        uint64_t n;
        uint8_t* dst;
        ow_item(a, bi, &p, &n, &dst);
        const ptrdiff_t dd = dst - p;
        uint64_t delta;
        if (n < 64 || (dd & 15) == 0) {
            delta = ow_reg64<G, U, true>(lds, p, n, dd, gl, lane, la);
        } else {
            delta = ow_reg64<G, 1, false>(lds, dst, n, 0, gl, lane, la);
            delta ^= ow_reg64<G, 1, false>(lds, p, n, 0, gl, lane, la);
            // the first lane's value (it alone walked the tails) to the group
            const uint32_t all = group_xor<G>(gl == 0 ? (uint32_t)delta ^ (uint32_t)(delta >> 32) : 0u);
            group_copy<G>(p, dst, n, ow_after(gl, all));
        }
        if (bi < a.count && gl == 0) a.out[bi] = delta;
    }
}

// photon_crc32c_patch_n / photon_crc64ecma_patch_n: a workgroup per target
// (targets beyond the grid: a stride loop), the target's writes round robin
// over its threads (patch_thread), the threads' values XORed over the wave
// and over the waves (LDS), thread 0 stores. Plain loads and stores only;
// nothing but out[m] is written. The workgroup is 64, 256 or 1,024 threads
// (the host picks by writes per target); a target with millions of writes is
// still one workgroup's work.
template <typename G, typename P>
__global__ __launch_bounds__(kFoldMaxBlock) void patch_kernel(const typename G::T* delta, const uint64_t* tail,
                                                              uint64_t nwrites, const uint64_t* tgt_start,
                                                              uint64_t ntgt, const typename G::T* in,
                                                              typename G::T* out, P pt) {
    typedef typename G::T T;
    __shared__ T red[kFoldMaxBlock / 64];
    const uint32_t t = threadIdx.x, nt = blockDim.x;
    for (uint64_t m = blockIdx.x; m < ntgt; m += gridDim.x) {  // m, s0, s1: the same on every thread
        uint64_t s0, s1;
        patch_bounds(tgt_start, nwrites, m, &s0, &s1);
        const T x = wave_xor(patch_thread<G>(delta, tail, s0, s1, t, nt, pt.x8pow2));
        if ((t & 63u) == 0) red[t >> 6] = x;
        __syncthreads();
        if (t == 0) {
            T all = in[m];
            for (uint32_t w = 0; w < nt / 64; ++w) all ^= red[w];
            out[m] = all;
        }
        __syncthreads();  // red is written again for the next target
    }
}

}  // namespace pcrc
