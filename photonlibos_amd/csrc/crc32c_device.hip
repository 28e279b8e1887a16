// crc32c_device.hip -- MI355X (gfx950) CRC32C engine behind the C-ABI of
// include/photon_crc/crc32c_gpu.h.
//
// What it computes: PhotonLibOS's raw CRC-32C, crc32c_extend(data, n, seed)
// (reference common/checksum/crc32c.h:30-33; engines crc.cpp:114-117,
// 339-368), for batches of independent device-resident buffers.
//
// How (DESIGN.md "Kernel"): a group of G lanes (G = 64: one wavefront per
// buffer; G < 64 packs 64/G small buffers per wavefront) walks the buffer in
// rows of G 16-byte blocks: lane l of the group loads block (row*G + l) with
// one coalesced global_load_dwordx4, so a row is one contiguous 16*G-byte
// sweep. Each lane keeps a partial CRC P over "its" column of blocks, as if
// the other lanes' bytes were zeros:
//     P <- P * x^(8*16*G) mod P  XOR  crc16(block)
// crc16(block) (the CRC of the 16 bytes alone) does not depend on P, so the
// U blocks a lane holds are reduced in parallel and only the cheap shift is
// on the loop-carried chain. All GF(2) products by constants are byte-sliced
// LDS table lookups (no carry-less multiply on CDNA4, no MFMA: this is GF(2)):
//   D tables: x -> x * x^32 mod P and S tables: P -> P * x^(8*16*G) mod P,
//             4 byte slices x 8 replicas each, 64 KiB together; lanes take
//             the slices in a per-lane rotated order so the 32 lanes of a
//             ds_read group always hit 32 distinct banks (crc32c_kernels.h).
// At the end lane l multiplies its partial by x^(128*d_l), d_l = number of
// 16-byte blocks between its last block and the end (byte-sliced R_k tables
// of x^(128*2^k) on the bits of d_l), and the group XOR-reduces with
// __shfl_xor.
// Unaligned heads use zero-prefix invariance (crc.md:24-32): the leading
// bytes of the first aligned block are masked to 0 and the seed is XORed into
// the first four data bytes (init-value linearity), so every load is an
// aligned 16-byte load. Ragged tails (<16 B) are finished byte-serially.
// (The streaming and fused variants of rounds 1-4 measured slower and were
// deleted in round 6; DESIGN.md §4 keeps their numbers.)
#include <hip/hip_runtime.h>

#include <errno.h>
#include <fcntl.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <sys/prctl.h>
#include <unistd.h>

#include <atomic>
#include <chrono>
#include <memory>
#include <map>
#include <tuple>
#include <mutex>
#include <string>
#include <thread>
#include <type_traits>
#include <vector>

#include <photon/common/checksum/crc32c.h>
#include <photon/common/checksum/crc64ecma.h>

#include "../../include/photon_crc/crc32c_gpu.h"
#include "../../include/photon_crc/tuning.h"
#include "crc32c_kernels.h"
#include "crc64_kernels.h"
#include "overwrite_kernels.h"
#include "xor_kernels.h"
#include "long_plan.h"
#include "multi_device.h"
#include "host_chunks.h"
#include "gf2.h"
#include "internal.h"

namespace pcrc {
int host_engine_table(int which, uint32_t* out, int n);  // crc32c_cpu.cpp

// ------------------------------------------------------------------ host side
namespace {

thread_local std::string g_err;

// Tuning knobs (include/photon_crc/tuning.h). Photon calls the checksum from
// many vCPU threads at once and the reference promises reentrant calls
// (crc.cpp:126-137: pointers written once, pure functions), so every knob is
// an atomic word that a launch reads ONCE; a multi-field shape (the long
// kernel's lanes and rounds) is packed into one word so a launch never sees
// half of a concurrent setter's update.
std::atomic<int> g_lanes_override{0};
// Workgroups of the persistent batch grids (photon_crc_set_batch_grid,
// tuning): 0 = one per CU (the default).
std::atomic<int> g_grid_cap{0};
// Rows per step of the generic batch kernel: -1 = by lane-group size
// (batch_rows), else 2, 4 or 8.
std::atomic<int> g_generic_u{-1};
// Rows per step of the one-kernel message form: 2 measured better than 4 on
// C5 (64 Ki messages x 8 x 8 KiB: +0.35 points per-segment, +0.8 chained)
// while strided batches keep 4 (C2 -6, C3 -1.2, C4 -0.9 with 2).
std::atomic<int> g_msg_u{2};
std::atomic<int> g_msg_mode{0};  // messages: 0 automatic, 1 one fused kernel, 2 segment kernel + fold kernel
// CRC-64 whole-step uniform batches: rows per step << 4 | mode (0 = the
// generic kernel, 1 = crc64_full_kernel, 2 = with the next buffer's first
// step prefetched across the finish, 3 = automatic: mode 2 for lane groups
// of up to 16 lanes, i.e. buffers up to 8 KiB, else the generic kernel;
// DESIGN.md §4.1).
std::atomic<uint32_t> g_full64{2u << 4 | 3u};
// Routed drop-in calls: spin window in µs | sleep-ahead << 16 (wait_tagged).
std::atomic<uint32_t> g_routed_wait{40u | 1u << 16};
// Resident small-buffer services (crc32c_small_service_kernel,
// crc64_small_service_kernel): idle time in µs after which a launch ends, 0
// = off (a launch per routed call). Default 200 µs; the environment variable
// PHOTON_CRC_SMALL_SERVICE (read at load) sets another value.
constexpr int kSvcIdleDefault = 200;
int svc_idle_from_env() {
    const char* e = getenv("PHOTON_CRC_SMALL_SERVICE");
    if (!e || !*e) return kSvcIdleDefault;
    const long v = strtol(e, nullptr, 10);
    return v < 0 ? 0 : v > 1000000 ? 1000000 : (int)v;
}
std::atomic<int> g_svc_idle_us{svc_idle_from_env()};
// Life of one service launch in µs (photon_crc_set_small_service_life): under
// steady traffic a launch ends after it and the next call starts another, so a
// caller's device-wide wait (hipDeviceSynchronize, hipFree) stalls at most
// this long behind it. 2 ms: one relaunch (~10 µs) per 2 ms of traffic.
std::atomic<int> g_svc_life_us{2000};
// The doorbell: 1 = device memory written through the PCIe BAR when the host
// mapping was verified (the default), 0 = the pinned host area (also with
// PHOTON_CRC_SVC_DOORBELL=host at load); photon_crc_set_service_doorbell.
int svc_bell_from_env() {
    const char* e = getenv("PHOTON_CRC_SVC_DOORBELL");
    return e && (!strcmp(e, "host") || !strcmp(e, "pinned") || !strcmp(e, "0")) ? 0 : 1;
}
std::atomic<int> g_svc_bell{svc_bell_from_env()};
std::atomic<uint64_t> g_svc_served{0}, g_svc_starts{0}, g_svc_missed{0}, g_svc_deferred{0};
std::atomic<int> g_svc_made{0};  // services created in this process (HeavyLaunch's fast path)
void service_end_all();  // (below) end every running service launch
// (below) before a batch, message or long launch of this library: end the
// running small-buffer services of the current device, so the launch never
// waits for their idle time
void svc_yield();
// (below) after such a launch: note it in the device's ring of heavy-launch
// events, which a routed call reads before it starts a service launch
void heavy_mark(hipStream_t st);

// A batch / message / long launch and the resident services never share the
// chip. Its workgroups (4 waves per SIMD at up to 120 VGPRs, 100-158 KiB of
// LDS) and a service's (100-126 VGPRs a wave) do not fit on one CU together,
// so a service beside a persistent one-workgroup-per-CU grid holds 33 of its
// workgroups off their CUs: C2 measured 0.83-0.97 ms per launch beside an idle
// service against 0.62-0.65 alone (repo:profiles/r06b_power_coresident.jsonl).
// So the launch ends the services first (svc_yield), and marks itself in the
// ring (heavy_mark) that keeps routed calls from starting a new service launch
// until it has finished -- those calls take the launch path meanwhile.
struct HeavyLaunch {
    hipStream_t st;
    explicit HeavyLaunch(hipStream_t s) : st(s) { svc_yield(); }
    ~HeavyLaunch() { heavy_mark(st); }
};
// (below) 1 = the device's service of this kind rings a BAR doorbell, 0 =
// the pinned one, -ENOENT = no service created yet
int service_doorbell_of(int dev, int kind);

int fail(int code, const std::string& what) {
    g_err = what;
    return code;
}

// what + rest: a kernel's name prefix (Crc32c::kKernel, Crc64::kKernel) and
// the rest of the text, joined only when there is an error to report.
int hip_fail(hipError_t e, const char* what, const char* rest = "") {
    return fail(-EIO, std::string(what) + rest + ": " + hipGetErrorString(e));
}

// The device runtime of multi_device.h.
struct HipRT {
    int get(int* dev) {
        const hipError_t e = hipGetDevice(dev);
        return e == hipSuccess ? 0 : hip_fail(e, "hipGetDevice");
    }
    int set(int dev) {
        const hipError_t e = hipSetDevice(dev);
        return e == hipSuccess ? 0 : hip_fail(e, "hipSetDevice");
    }
};

struct DeviceInfo {
    bool probed = false;
    bool ok = false;
    int cus = 0;
};

std::mutex g_mu;
std::vector<DeviceInfo> g_dev;
thread_local int g_fail_next = 0;  // photon_crc_test_fail_next (tuning.h)

void table_images_init();  // (below) the device's table-prologue images

// Resolve the current device; only gfx950 is supported (no other code path).
// Every device entry point passes through here before it enqueues anything.
int current_device(int* cus) {
    if (g_fail_next > 0) {
        --g_fail_next;
        return fail(-EIO, "injected failure (photon_crc_test_fail_next)");
    }
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return hip_fail(e, "hipGetDevice");
    std::lock_guard<std::mutex> lk(g_mu);
    if ((int)g_dev.size() <= dev) g_dev.resize(dev + 1);
    DeviceInfo& di = g_dev[dev];
    if (!di.probed) {
        hipDeviceProp_t prop;
        e = hipGetDeviceProperties(&prop, dev);
        if (e != hipSuccess) return hip_fail(e, "hipGetDeviceProperties");
        di.ok = strncmp(prop.gcnArchName, "gfx950", 6) == 0;
        di.cus = prop.multiProcessorCount;
        di.probed = true;
        if (!di.ok) g_err = std::string("device is ") + prop.gcnArchName + ", need gfx950";
        if (di.ok) table_images_init();
    }
    if (!di.ok) return fail(-ENODEV, "photon_crc: no gfx950 device (got other arch)");
    *cus = di.cus;
    return dev;
}

// Scratch for multi-kernel calls (segment CRCs between the segment and fold
// kernels, piece descriptors of one long buffer). NOT from HIP's stream-ordered
// allocator: with 16 threads submitting on their own streams, hipMallocAsync /
// hipFreeAsync on the default pool handed one call's segment-CRC scratch to
// another stream now and then (2-8 wrong message CRCs in 30 K,
// tests/cpp/concurrency_test.cpp), and a private pool with cross-stream reuse
// off hung the process about one run in four. Instead the library keeps its
// own device buffers: a call leases a buffer that no other call holds, makes
// its stream wait for the event recorded after the buffer's previous use
// (usually complete already: leases prefer such buffers), enqueues its work,
// records the event again and returns the lease. Reuse across streams is
// ordered by that event; nothing is freed while work may still use it.
struct ScratchBuf {
    int dev;
    void* p;
    uint64_t cap;
    hipEvent_t last;  // recorded after the latest use
    bool busy;
    bool zeroed;      // a state buffer: zero when created, and every user leaves it zero
};
std::mutex g_scr_mu;
std::vector<ScratchBuf*> g_scr;
int64_t scratch_trim_locked(bool all);

// zeroed: a small state buffer (the long-buffer kernel's accumulator and
// ticket) that is zero when leased; the kernel that uses it leaves it zero.
int scratch_alloc(void** p, uint64_t bytes, hipStream_t st, bool zeroed = false) {
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return hip_fail(e, "hipGetDevice");
    ScratchBuf* lease = nullptr;
    bool wait = false;
    {
        std::lock_guard<std::mutex> lk(g_scr_mu);
        (void)scratch_trim_locked(false);
        for (ScratchBuf* b : g_scr) {
            if (b->busy || b->dev != dev || b->cap < bytes || b->zeroed != zeroed) continue;
            const bool done = hipEventQuery(b->last) == hipSuccess;
            if (!lease || (done && wait)) {
                lease = b;
                wait = !done;
            }
            if (done) break;
        }
        if (lease) lease->busy = true;
    }
    if (!lease) {
        auto* b = new ScratchBuf{dev, nullptr, 0, nullptr, true, zeroed};
        uint64_t cap = zeroed ? 256u : 1u << 20;
        while (cap < bytes) cap <<= 1;
        if ((e = hipMalloc(&b->p, cap)) != hipSuccess) {
            delete b;
            return hip_fail(e, "hipMalloc(scratch)");
        }
        // stream-ordered before its first use on `st`: a plain hipMemset runs on
        // the null stream, which does not order against non-blocking streams
        // (the zeroing of a reduce state landed after the first kernel that
        // used it: scripts/soak_service.py)
        if (zeroed && (e = hipMemsetAsync(b->p, 0, cap, st)) != hipSuccess) {
            (void)hipFree(b->p);
            delete b;
            return hip_fail(e, "hipMemset(state)");
        }
        if ((e = hipEventCreateWithFlags(&b->last, hipEventDisableTiming)) != hipSuccess) {
            (void)hipFree(b->p);
            delete b;
            return hip_fail(e, "hipEventCreate(scratch)");
        }
        b->cap = cap;
        std::lock_guard<std::mutex> lk(g_scr_mu);
        g_scr.push_back(b);
        lease = b;
    } else if (wait && (e = hipStreamWaitEvent(st, lease->last, 0)) != hipSuccess) {
        std::lock_guard<std::mutex> lk(g_scr_mu);
        lease->busy = false;
        return hip_fail(e, "hipStreamWaitEvent(scratch)");
    }
    *p = lease->p;
    return 0;
}

// Buffers kept for reuse are capped (a buffer used to keep the
// size of the largest request it ever served for the life of the process):
// an idle buffer above kScratchKeep bytes, or any idle buffer beyond
// kScratchMaxIdle bytes of idle scratch on its device, is freed by the next
// lease once its last use has completed. photon_crc_scratch_release() frees
// every idle buffer whose work has completed.
constexpr uint64_t kScratchKeep = 64ull << 20;
constexpr uint64_t kScratchMaxIdle = 256ull << 20;

// Free idle buffers whose last use has completed: all of them (`all`), or the
// oversized ones and those beyond the idle cap. Caller holds g_scr_mu.
int64_t scratch_trim_locked(bool all) {
    int64_t freed = 0;
    std::vector<uint64_t> idle_dev(64, 0);
    for (auto it = g_scr.begin(); it != g_scr.end();) {
        ScratchBuf* b = *it;
        const bool idle = !b->busy && hipEventQuery(b->last) == hipSuccess;
        uint64_t& kept = idle_dev[b->dev & 63];
        if (idle && (all || b->cap > kScratchKeep || kept + b->cap > kScratchMaxIdle)) {
            (void)hipEventDestroy(b->last);
            services_end_before_free();
            (void)hipFree(b->p);
            freed += (int64_t)b->cap;
            delete b;
            it = g_scr.erase(it);
            continue;
        }
        if (idle) kept += b->cap;
        ++it;
    }
    return freed;
}

// Return a lease: its buffer may be reused once the work enqueued on `st`
// so far has run.
int scratch_free(void* p, hipStream_t st) {
    ScratchBuf* lease = nullptr;
    {
        std::lock_guard<std::mutex> lk(g_scr_mu);
        for (ScratchBuf* b : g_scr)
            if (b->p == p && b->busy) lease = b;
    }
    if (!lease) return fail(-EINVAL, "scratch_free of a buffer not leased");
    const hipError_t e = hipEventRecord(lease->last, st);
    if (e != hipSuccess) return hip_fail(e, "hipEventRecord(scratch)");  // stays leased: never reused unordered
    std::lock_guard<std::mutex> lk(g_scr_mu);
    lease->busy = false;
    return 0;
}

// Constants for G lanes per buffer and runs of B blocks per lane per row:
// row shift x^(8*16*B*G), lane-combine basis of x^(8*16*B*2^k).
LaneConsts make_lane_consts(int g, int b) {
    LaneConsts c;
    c.kshift = xpow(8ull * 16ull * (uint64_t)b * (uint64_t)g);
    mul_basis(c.kshift, c.sbasis);
    for (int k = 0; k < 6; ++k) mul_basis(xpow((128ull * (uint64_t)b) << k), c.basis[k]);
    for (int d = 0; d < 8; ++d) mul_basis(xpow(32ull + 128ull * (uint64_t)d), c.fbasis[d]);
    return c;
}

const LaneConsts& lane_consts(int g, int b = 1) {
    static LaneConsts tab[7][3];
    static std::once_flag once;
    std::call_once(once, [] {
        for (int lg = 2; lg <= 6; ++lg)
            for (int lb = 0; lb <= 2; ++lb) tab[lg][lb] = make_lane_consts(1 << lg, 1 << lb);
    });
    const int lg = g == 64 ? 6 : g == 32 ? 5 : g == 16 ? 4 : g == 8 ? 3 : 2;
    const int lb = b == 4 ? 2 : b == 2 ? 1 : 0;
    return tab[lg][lb];
}

LaneConsts64 make_lane_consts64(int g) {
    LaneConsts64 c;
    c.kshift = xpow64(8ull * 16ull * (uint64_t)g);
    for (int i = 0; i < 64; ++i) c.sbasis[i] = mulmod64(1ull << i, c.kshift);
    return c;
}

const LaneConsts64& lane_consts64(int g) {
    static LaneConsts64 tab[7];
    static std::once_flag once;
    std::call_once(once, [] {
        for (int lg = 2; lg <= 6; ++lg) tab[lg] = make_lane_consts64(1 << lg);
    });
    return tab[g == 64 ? 6 : g == 32 ? 5 : g == 16 ? 4 : g == 8 ? 3 : 2];
}

// The power tables of width W (Crc32c or Crc64, below): t[i] = v^(2^i), 64
// successive squarings of v.
template <typename W>
typename W::Pow squarings(typename W::T v) {
    typename W::Pow t;
    for (int i = 0; i < 64; ++i) {
        t.x8pow2[i] = v;
        v = W::mul(v, v);
    }
    return t;
}

// x^(8*2^i), or with INV x^(-8*2^i), built once.
template <typename W, bool INV>
const typename W::Pow& x8_table() {
    static typename W::Pow t;
    static std::once_flag once;
    std::call_once(once, [] { t = squarings<W>(INV ? W::xpow_inv(8) : W::xpow(8)); });
    return t;
}

template <typename W>
const typename W::Pow& pow_table() {
    return x8_table<W, false>();
}

// x^(-8*2^i): the right shift of crc32c_rshift_sw (crc_tables.cpp:147-164).
template <typename W>
const typename W::Pow& rshift_table() {
    return x8_table<W, true>();
}

// x^(8*part*2^i): powers of K = x^(8*part) for the combine_series kernels
// (CRC-64 with part 0: K = 1).
template <typename W>
typename W::Pow part_pow_table(uint64_t part) {
    return squarings<W>(W::xpow(8ull * part));
}

// Lanes per buffer: one wavefront per buffer for large buffers; pack small
// buffers so every lane still walks >= 16 rows (DESIGN.md "Lane groups").
int choose_lanes(uint64_t typical_len) {
    if (const int g = g_lanes_override.load(std::memory_order_relaxed)) return g;
    // Measured with scripts/tune_gpu.py (profiles/tune_r01.md): 1 MiB buffers
    // G=64, 64 KiB G=32, 4-8 KiB G=8.
    if (typical_len >= (512u << 10)) return 64;
    if (typical_len >= (32u << 10)) return 32;
    if (typical_len >= 2048) return 8;
    return 4;
}

// Lane-group size of the CRC32C generic batch kernel: as choose_lanes, but
// 4-8 KiB buffers take 16 lanes (with 2 rows per step, batch_rows): C3 (1 Mi x
// 4 KiB) 85.5 % vs 83.7 % for 8 lanes x 4 rows (profiles/r02_tune_lanes_rows.jsonl).
int batch_lanes(uint64_t typical_len) {
    if (const int g = g_lanes_override.load(std::memory_order_relaxed)) return g;
    if (typical_len >= 4096 && typical_len < 8192) return 16;
    return choose_lanes(typical_len);
}

// The default rows per step of a lane-group size.
constexpr int default_rows(int g) { return g == 16 ? 2 : 4; }

int batch_rows(int g) {
    const int u = g_generic_u.load(std::memory_order_relaxed);
    return u >= 0 ? u : default_rows(g);
}

std::vector<uint32_t> small_image_host();    // (below) the small kernels' table images
std::vector<uint64_t> small64_image_host();

// The two CRC widths. The host paths below are written once, as templates over
// one of these structs; whatever differs between CRC-32C and CRC-64/ECMA on
// the host side is a member here (or a pair of overloads on the kernels'
// argument structs, for the launchers), never a branch inside a shared body.
// Gf32 / Gf64 (fold_parts.h) give the word type T and mul() = mulmod.
struct Crc32c : Gf32 {
    static constexpr const char* kKernel = "crc32c";  // the kernels' name prefix, for error texts
    static constexpr const char* kExtend = "crc32c_extend";  // the drop-in calls, for routed failures
    static constexpr const char* kSeries = "crc32c_series";
    static constexpr const char* kCombineSeries = "crc32c_combine_series";
    static constexpr const char* kCombineSeriesLaunch = "combine_series kernel launch";
    static constexpr bool kCrc64 = false;  // long_plan_for / long_powers
    static constexpr int kService = 0;     // service_small's kind
    typedef LaneConsts Lanes;
    typedef PowTable Pow;
    typedef BatchArgs Batch;
    typedef CopyBatchArgs CopyBatch;
    typedef CopyIovArgs CopyIov;
    typedef SmallArgs Small;
    typedef LongArgs Long;
    typedef CopyLongArgs CopyLong;
    static T xpow(uint64_t n) { return pcrc::xpow(n); }
    static T xpow_inv(uint64_t n) { return pcrc::xpow_inv(n); }
    static const Lanes& lanes(int g) { return lane_consts(g); }
    // Uniform aligned batches start from seed0 * x^(8 nbytes) (crc32c_kernels.h shift_init).
    static constexpr bool kShiftInit = PCRC_SHIFT_INIT;
    static T shift_init(T seed0, uint64_t nbytes) { return mul(seed0, xpow(8ull * nbytes)); }
    // Strided and iovec copies take the lanes of the plain batch (batch_lanes:
    // 16 lanes for 4-8 KiB).
    static int copy_lanes(uint64_t typical_len) { return batch_lanes(typical_len); }
    // crc32c_series_hw (crc.cpp:481-500) leaves parts below 8 bytes at 0.
    static constexpr uint32_t kSeriesMinPart = 8;
    // The small kernel: the seed's 4 bytes lie inside the grid; stored as given.
    static constexpr uint32_t kSeedBytes = 4;
    static void put_seed(Small* a, T seed) { a->seed = seed; }
    static T seed_word(const Small& a) { return a.seed; }
    static constexpr uint32_t kImageBytes = kSmImage;
    static constexpr const char* kImageName = "small-buffer table image";
    static std::vector<T> image_host() { return small_image_host(); }
    static constexpr uint32_t kMidBlocks = pcrc::kMidBlocks, kMidRows = pcrc::kMidRows;
    template <uint32_t V, int R>
    static auto small_kernel() { return &crc32c_small_kernel<V, R>; }
    template <int G>
    static auto long_kernel() { return &crc32c_long_kernel<G, 4>; }
    template <int G>
    static auto copy_long_kernel() { return &crc32c_copy_long_kernel<G, 4>; }
    static void long_args(Long* a, const LongPlan& lp, const LongPowers& pw, const void* data, T seed, T* out) {
        pcrc::long_args(a, lp, pw, data, seed, out);
    }
    static constexpr auto* kCombineKernel = &crc32c_combine_kernel;
    static constexpr auto* kTrimKernel = &crc32c_trim_kernel;
    static constexpr auto* kFoldPartsKernel = &crc32c_fold_parts_kernel;
    typedef PartsArgs Parts;
    template <int G, bool COPY>
    static auto parts_kernel() { return &crc32c_parts_kernel<G, default_rows(G), COPY>; }
    static constexpr auto* kPartsFoldKernel = &crc32c_parts_fold_kernel;
    static constexpr const char* kPartsFoldLaunch = "crc32c_parts_fold_kernel launch";
    typedef PartsPackedArgs PartsPacked;
    template <int G, bool COPY>
    static auto parts_packed_kernel() { return &crc32c_parts_packed_kernel<G, default_rows(G), COPY>; }
    static constexpr auto* kPartsPackedFoldKernel = &crc32c_parts_packed_fold_kernel;
    static constexpr const char* kPartsPackedFoldLaunch = "crc32c_parts_packed_fold_kernel launch";
    static constexpr auto* kCombineSeriesKernel = &crc32c_combine_series_kernel;
    // combine_series over empty parts: crc32c_combine_series_hw/sw return the
    // first nonzero part CRC (a kernel of its own). true = launched.
    static bool combine_series_of_empty(const T* d_crc, uint32_t part_size, uint32_t n_parts, T* d_result,
                                        hipStream_t st) {
        if (part_size) return false;
        hipLaunchKernelGGL(crc32c_first_nonzero_kernel, dim3(1), dim3(1024), 0, st, d_crc, (uint64_t)n_parts,
                           d_result);
        return true;
    }
    // A routed result: one tagged word per workgroup (small kernel) or one in
    // all (long_reduce), the CRC in its low half.
    static constexpr uint32_t kWords = 1;
    static T routed_result(const uint32_t* x, bool /*raw*/) { return x[0]; }
    static void routed_diag(char* buf, size_t n, const volatile uint64_t* w, uint32_t tag) {
        snprintf(buf, n, "; word %016llx, tag %08x", (unsigned long long)w[0], tag);
    }
    // The host engines saved from the drop-in pointers (written before the
    // routed pointers are published, see photon_crc_set_device_dispatch).
    static inline T (*host_crc)(const uint8_t*, size_t, T) = nullptr;
    static inline void (*host_series)(const uint8_t*, uint32_t, uint32_t, T*) = nullptr;
    static inline T (*host_cseries)(T*, uint32_t, uint32_t) = nullptr;
};

struct Crc64 : Gf64 {
    static constexpr const char* kKernel = "crc64";
    static constexpr const char* kExtend = "crc64ecma_extend";
    static constexpr const char* kSeries = "crc64ecma_series";
    static constexpr const char* kCombineSeries = "crc64ecma_combine_series";
    static constexpr const char* kCombineSeriesLaunch = "crc64_combine_series_kernel launch";
    static constexpr bool kCrc64 = true;
    static constexpr int kService = 1;
    typedef LaneConsts64 Lanes;
    typedef PowTable64 Pow;
    typedef Batch64Args Batch;
    typedef CopyBatch64Args CopyBatch;
    typedef CopyIov64Args CopyIov;
    typedef Small64Args Small;
    typedef Long64Args Long;
    typedef CopyLong64Args CopyLong;
    static T xpow(uint64_t n) { return xpow64(n); }
    static T xpow_inv(uint64_t n) { return xpow64_inv(n); }
    static const Lanes& lanes(int g) { return lane_consts64(g); }
    // The register starts from the inverted seed (crc.cpp:119-122).
    static constexpr bool kShiftInit = PCRC64_SHIFT_INIT;
    static T shift_init(T seed0, uint64_t nbytes) { return mul(~seed0, xpow(8ull * nbytes)); }
    // Strided and iovec copies take choose_lanes as it is, without the 4-8 KiB
    // rule of the plain batch.
    static int copy_lanes(uint64_t typical_len) { return choose_lanes(typical_len); }
    // crc64ecma of no bytes is 0; every other part size is read (the host
    // engines have no short-part rule, crc64_cpu.cpp).
    static constexpr uint32_t kSeriesMinPart = 1;
    // The small kernel: the init's 8 bytes lie inside the grid; stored inverted.
    static constexpr uint32_t kSeedBytes = 8;
    static void put_seed(Small* a, T seed) { a->init = ~seed; }
    static T seed_word(const Small& a) { return a.init; }
    static constexpr uint32_t kImageBytes = kSm64Image;
    static constexpr const char* kImageName = "CRC-64 small-buffer table image";
    static std::vector<T> image_host() { return small64_image_host(); }
    static constexpr uint32_t kMidBlocks = kMid64Blocks, kMidRows = kMid64Rows;
    template <uint32_t V, int R>
    static auto small_kernel() { return &crc64_small_kernel<V, R>; }
    template <int G>
    static auto long_kernel() { return &crc64_long_kernel<G>; }
    template <int G>
    static auto copy_long_kernel() { return &crc64_copy_long_kernel<G>; }
    static void long_args(Long* a, const LongPlan& lp, const LongPowers& pw, const void* data, T seed, T* out) {
        long_args64(a, lp, pw, data, seed, out);
    }
    static constexpr auto* kCombineKernel = &crc64_combine_kernel;
    static constexpr auto* kTrimKernel = &crc64_trim_kernel;
    static constexpr auto* kFoldPartsKernel = &crc64_fold_parts_kernel;
    typedef Parts64Args Parts;
    // null: the copying form in an A/B build of the row loop (kCopying64)
    template <int G, bool COPY>
    static auto parts_kernel() {
        if constexpr (COPY && !kCopying64) return static_cast<void (*)(Parts64Args, LaneConsts64)>(nullptr);
        else return &crc64_parts_kernel<G, COPY>;
    }
    static constexpr auto* kPartsFoldKernel = &crc64_parts_fold_kernel;
    static constexpr const char* kPartsFoldLaunch = "crc64_parts_fold_kernel launch";
    typedef PartsPacked64Args PartsPacked;
    template <int G, bool COPY>
    static auto parts_packed_kernel() {
        if constexpr (COPY && !kCopying64) return static_cast<void (*)(PartsPacked64Args, LaneConsts64)>(nullptr);
        else return &crc64_parts_packed_kernel<G, COPY>;
    }
    static constexpr auto* kPartsPackedFoldKernel = &crc64_parts_packed_fold_kernel;
    static constexpr const char* kPartsPackedFoldLaunch = "crc64_parts_packed_fold_kernel launch";
    static constexpr auto* kCombineSeriesKernel = &crc64_combine_series_kernel;
    // No rule for empty parts: K = x^0 = 1 in crc64_combine_series_kernel.
    static bool combine_series_of_empty(const T*, uint32_t, uint32_t, T*, hipStream_t) { return false; }
    // A routed result: two tagged words, low and high half. The small kernel's
    // workgroups return raw values, which the host XORs and inverts
    // (crc.cpp:119-122); long_reduce has inverted its result already.
    static constexpr uint32_t kWords = 2;
    static T routed_result(const uint32_t* x, bool raw) {
        const T v = ((T)x[1] << 32) | x[0];
        return raw ? ~v : v;
    }
    static void routed_diag(char* buf, size_t n, const volatile uint64_t* w, uint32_t tag) {
        snprintf(buf, n, "; words %016llx %016llx, tag %08x", (unsigned long long)w[0], (unsigned long long)w[1],
                 tag);
    }
    static inline T (*host_crc)(const uint8_t*, size_t, T) = nullptr;
    static inline void (*host_series)(const uint8_t*, uint32_t, uint32_t, T*) = nullptr;
    static inline T (*host_cseries)(T*, uint32_t, uint32_t) = nullptr;
};

// The persistent grid of a batch launch: `units` buffers or messages, 64 / g
// of them per wavefront, kWaves wavefronts per workgroup, at most one
// workgroup per CU and, when `capped`, at most photon_crc_set_batch_grid's.
uint64_t batch_grid(uint64_t units, int g, int cus, bool capped) {
    const uint64_t gpw = 64 / (uint64_t)g;
    const uint64_t waves = (units + gpw - 1) / gpw;
    uint64_t grid = (waves + kWaves - 1) / kWaves;
    if (grid > (uint64_t)cus) grid = cus;
    if (capped)
        if (const int cap = g_grid_cap.load(std::memory_order_relaxed))
            grid = grid > (uint64_t)cap ? (uint64_t)cap : grid;
    return grid;
}

template <int N>
using Int = std::integral_constant<int, N>;

// The lane-group size as a compile-time constant: f(Int<G>{}).
template <typename F>
void with_lanes(int g, F f) {
    switch (g) {
        case 64: f(Int<64>{}); break;
        case 32: f(Int<32>{}); break;
        case 16: f(Int<16>{}); break;
        case 8: f(Int<8>{}); break;
        default: f(Int<4>{}); break;
    }
}

// One persistent launch over `units` buffers or messages in groups of g
// lanes: launch(Int<G>{}, grid, kc) enqueues the kernel build of G lanes.
template <typename W, typename L>
int launch_lanes(uint64_t units, int g, bool capped, hipStream_t stream, const char* what, L launch) {
    if (units == 0) return 0;
    int cus = 0;
    int dev = current_device(&cus);
    if (dev < 0) return dev;
    const dim3 grid(batch_grid(units, g, cus, capped));
    const typename W::Lanes& kc = W::lanes(g);
    HeavyLaunch heavy(stream);
    with_lanes(g, [&](auto G) { launch(G, grid, kc); });
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : hip_fail(e, what);
}

// lanes: 0 = by typical_len (batch_lanes), else the lane-group size.
int launch_batch(const BatchArgs& a, uint64_t typical_len, hipStream_t stream, int lanes = 0) {
    const int g = lanes ? lanes : batch_lanes(typical_len);
    const int rows_per_step = batch_rows(g);
    return launch_lanes<Crc32c>(a.count, g, true, stream, "crc32c_batch_kernel launch",
                                [&](auto G, dim3 grid, const LaneConsts& kc) {
        auto rows = [&](auto U) {
            hipLaunchKernelGGL((crc32c_batch_kernel<decltype(G)::value, decltype(U)::value>), grid, dim3(kBlock), 0,
                               stream, a, kc, pow_table<Crc32c>());
        };
        if (rows_per_step == 2)
            rows(Int<2>{});
        else if (rows_per_step == 8)
            rows(Int<8>{});
        else
            rows(Int<4>{});
    });
}

// The copying kernels (crc32c_batch_kernel<G, U, MSG, true>): one build per
// lane-group size, with the default rows per step of that size
// (photon_crc_set_generic_rows does not apply; photon_crc_set_lanes_per_buffer
// does). msg: 0 = buffers, 1 = messages chained, 2 = messages with per-segment
// CRCs; units = buffers or messages.
int launch_copy(const CopyBatchArgs& a, uint64_t units, int g, hipStream_t stream, int msg = 0) {
    return launch_lanes<Crc32c>(units, g, true, stream, "crc32c_batch_kernel<copy> launch",
                                [&](auto G, dim3 grid, const LaneConsts& kc) {
        constexpr int GG = decltype(G)::value, U = default_rows(GG);
        if (msg == 2)
            hipLaunchKernelGGL((crc32c_batch_kernel<GG, U, 2, true>), grid, dim3(kBlock), 0, stream, a, kc,
                               pow_table<Crc32c>());
        else if (msg == 1)
            hipLaunchKernelGGL((crc32c_batch_kernel<GG, U, 1, true>), grid, dim3(kBlock), 0, stream, a, kc,
                               pow_table<Crc32c>());
        else
            hipLaunchKernelGGL((crc32c_batch_kernel<GG, U, 0, true>), grid, dim3(kBlock), 0, stream, a, kc,
                               pow_table<Crc32c>());
    });
}

// crc32c_copy_iov_kernel<G, U>: one build per lane-group
// size with the default rows per step of that size, grid as launch_copy.
int launch_copy_iov(const CopyIovArgs& a, int g, hipStream_t stream) {
    return launch_lanes<Crc32c>(a.nmsg, g, true, stream, "crc32c_copy_iov_kernel launch",
                                [&](auto G, dim3 grid, const LaneConsts& kc) {
        constexpr int GG = decltype(G)::value;
        hipLaunchKernelGGL((crc32c_copy_iov_kernel<GG, default_rows(GG)>), grid, dim3(kBlock), 0, stream, a, kc);
    });
}

// crc32c_copy_iov_seg_kernel<G, U, DST>: as launch_copy_iov,
// one build per lane-group size and side.
int launch_copy_iov_seg(const CopyIovSegArgs& a, bool dst_side, int g, hipStream_t stream) {
    return launch_lanes<Crc32c>(a.nmsg, g, true, stream, "crc32c_copy_iov_seg_kernel launch",
                                [&](auto G, dim3 grid, const LaneConsts& kc) {
        constexpr int GG = decltype(G)::value, U = default_rows(GG);
        if (dst_side)
            hipLaunchKernelGGL((crc32c_copy_iov_seg_kernel<GG, U, true>), grid, dim3(kBlock), 0, stream, a, kc,
                               pow_table<Crc32c>());
        else
            hipLaunchKernelGGL((crc32c_copy_iov_seg_kernel<GG, U, false>), grid, dim3(kBlock), 0, stream, a, kc,
                               pow_table<Crc32c>());
    });
}

// The CRC-64 plain batch. Unlike launch_batch above it picks its lanes with
// choose_lanes and the 4-8 KiB rule below, takes the full-row kernel for
// whole-step uniform batches (g_full64), and has no rows knob.
int launch_batch(const Batch64Args& a, uint64_t typical_len, hipStream_t stream) {
    int g = choose_lanes(typical_len);
    const uint32_t full = g_full64.load(std::memory_order_relaxed);
    // rows per step: automatic mode 4 rows for buffers of 8 KiB and more (8
    // KiB: 0.832 vs 0.823 at the power limit), 2 below (4 KiB: 0.809 vs 0.804;
    // repo:profiles/r06n_power_crc64_rows_*.jsonl); else the knob's
    const int fu = (full & 15u) == 3u ? (typical_len >= 8192 ? 4 : 2) : (int)(full >> 4);
    auto full_rows = [&](int gg) {  // the full-row kernel's mode for lane groups of gg, 0 = not eligible
        const int fx = (full & 15u) == 3u ? (gg <= 16 ? 2 : 0) : (int)(full & 15u);
        return fx && !a.iov && a.shift_init && a.nbytes % (2ull * 16ull * (uint64_t)gg * (uint64_t)fu) == 0 ? fx : 0;
    };
    // 4-8 KiB CRC-64 buffers: the full-row kernel takes 8 lanes (32-64 rows
    // per lane, so the per-buffer finish -- 16 nibble lookups per lane -- is
    // spread over twice the bytes of 16 lanes): at the board's power limit
    // 4 KiB 0.802 vs 0.796 of 8 TB/s (0.2344 vs 0.2360 J/GiB), 8 KiB 0.817
    // vs 0.784 (0.2297 vs 0.2404), bench C3 shape 0.795 vs 0.786
    // (repo:profiles/r06c_power_crc64_lanes_g{16,8}.jsonl, r06c_ab_lanes_c3_crc64.jsonl).
    // Other batches there keep 16 lanes (the generic kernel: 80.7 vs 79.8 %,
    // repo:profiles/r04_ab_crc64_c3_lanes8_vs_16.jsonl).
    if (!g_lanes_override.load(std::memory_order_relaxed) && typical_len >= 4096 && typical_len <= 8192)
        g = full_rows(8) ? 8 : 16;
    // Whole-step uniform batches: the full-row kernel (crc64_kernels.h).
    const int fx = full_rows(g);
    // capped = false: photon_crc_set_batch_grid does not apply to the plain
    // CRC-64 batch (this launcher "is as it was").
    return launch_lanes<Crc64>(a.count, g, false, stream, fx ? "crc64_full_kernel launch" : "crc64_batch_kernel launch",
                               [&](auto G, dim3 grid, const LaneConsts64& kc) {
        constexpr int GG = decltype(G)::value;
        auto full = [&](auto U) {
            constexpr int UU = decltype(U)::value;
            if (fx == 2)
                hipLaunchKernelGGL((crc64_full_kernel<GG, UU, true>), grid, dim3(kBlock), 0, stream, a, kc);
            else
                hipLaunchKernelGGL((crc64_full_kernel<GG, UU, false>), grid, dim3(kBlock), 0, stream, a, kc);
        };
        if (!fx)
            hipLaunchKernelGGL(crc64_batch_kernel<GG>, grid, dim3(kBlock), 0, stream, a, kc);
        else if (fu == 4)
            full(Int<4>{});
        else
            full(Int<2>{});
    });
}

// launch_lanes for the CRC-64 copying kernels.
template <typename L>
int launch_copying64(uint64_t units, int g, hipStream_t stream, const char* what, L launch) {
#if PCRC64_ABL != 0 || PCRC64_ROLL != 1 || PCRC64_U != 2
    // A/B builds of the row loop: the copying kernels exist for the product's loop only
    (void)launch;
    return units == 0 ? 0 : fail(-ENOTSUP, "the copying CRC-64 kernels are not part of this A/B build");
#else
    return launch_lanes<Crc64>(units, g, true, stream, what, launch);
#endif
}

// The CRC-64 copying kernels (crc64_batch_kernel<G, true>, crc64_gather_kernel<G>;
// DESIGN.md §4.4): always the generic kernel, one build per lane-group size
// (photon_crc_set_lanes_per_buffer and photon_crc_set_batch_grid apply; the
// full-row kernel has no copying form). gather: units = messages.
int launch_copy(const CopyBatch64Args& a, uint64_t units, int g, hipStream_t stream, bool gather = false) {
    return launch_copying64(units, g, stream, gather ? "crc64_gather_kernel launch" : "crc64_batch_kernel<copy> launch",
                            [&](auto G, dim3 grid, const LaneConsts64& kc) {
        constexpr int GG = decltype(G)::value;
        if (gather)
            hipLaunchKernelGGL((crc64_gather_kernel<GG>), grid, dim3(kBlock), 0, stream, a, kc);
        else
            hipLaunchKernelGGL((crc64_batch_kernel<GG, true>), grid, dim3(kBlock), 0, stream, a, kc);
    });
}

// The overwrite + delta kernels (crc32c_overwrite_kernel<G, U>,
// crc64_overwrite_kernel<G, U>): one build per lane-group
// size with overwrite_rows(G) rows per step (the rows knobs do not apply;
// photon_crc_set_lanes_per_buffer and photon_crc_set_batch_grid do).
// Two streams in flight cost 8 VGPRs per row where the copy's one costs 4:
// 2 rows per step at every lane-group size keep every build inside the 128
// VGPRs of one 1,024-thread workgroup per CU without scratch.
#ifndef PCRC_OW_ROWS  // A/B builds (the Makefile's EXTRA): 4
#define PCRC_OW_ROWS 2
#endif
constexpr int overwrite_rows(int /*g*/) { return PCRC_OW_ROWS; }

int launch_overwrite(const OverwriteArgs<uint32_t>& a, int g, hipStream_t stream) {
    return launch_lanes<Crc32c>(a.count, g, true, stream, "crc32c_overwrite_kernel launch",
                                [&](auto G, dim3 grid, const LaneConsts& kc) {
        constexpr int GG = decltype(G)::value;
        hipLaunchKernelGGL((crc32c_overwrite_kernel<GG, overwrite_rows(GG)>), grid, dim3(kBlock), 0, stream, a, kc);
    });
}

int launch_overwrite(const OverwriteArgs<uint64_t>& a, int g, hipStream_t stream) {
    return launch_lanes<Crc64>(a.count, g, true, stream, "crc64_overwrite_kernel launch",
                               [&](auto G, dim3 grid, const LaneConsts64& kc) {
        constexpr int GG = decltype(G)::value;
        hipLaunchKernelGGL((crc64_overwrite_kernel<GG, overwrite_rows(GG)>), grid, dim3(kBlock), 0, stream, a, kc);
    });
}

// The stripe parity + CRC kernels (crc32c_xor_kernel<G, U>, crc64_xor_kernel<G, U>;
// DESIGN.md §4.16): one build per lane-group size (the rows knobs do not apply;
// photon_crc_set_lanes_per_buffer and photon_crc_set_batch_grid do). A row
// costs 4 VGPRs of accumulator and 4 * kXorInFlight of loads in flight. With 4
// loads in flight the CRC-32C builds take 2 rows per step (85 to 115 VGPRs);
// the CRC-64 builds, whose table steps hold twice the registers, spill at 2
// rows for every lane group below 64 and take 1 (89 to 111 VGPRs): every build
// stays inside the 128 VGPRs of one 1,024-thread workgroup per CU without
// scratch.
#ifndef PCRC_XOR_ROWS  // A/B builds (the Makefile's EXTRA)
#define PCRC_XOR_ROWS 2
#endif
#ifndef PCRC_XOR_ROWS64
#define PCRC_XOR_ROWS64 1
#endif
constexpr int xor_rows(int /*g*/) { return PCRC_XOR_ROWS; }
constexpr int xor_rows64(int /*g*/) { return PCRC_XOR_ROWS64; }

int launch_xor(const XorArgs<uint32_t>& a, int g, hipStream_t stream) {
    return launch_lanes<Crc32c>(a.count, g, true, stream, "crc32c_xor_kernel launch",
                                [&](auto G, dim3 grid, const LaneConsts& kc) {
        constexpr int GG = decltype(G)::value;
        hipLaunchKernelGGL((crc32c_xor_kernel<GG, xor_rows(GG)>), grid, dim3(kBlock), 0, stream, a, kc);
    });
}

int launch_xor(const XorArgs<uint64_t>& a, int g, hipStream_t stream) {
    return launch_lanes<Crc64>(a.count, g, true, stream, "crc64_xor_kernel launch",
                               [&](auto G, dim3 grid, const LaneConsts64& kc) {
        constexpr int GG = decltype(G)::value;
        hipLaunchKernelGGL((crc64_xor_kernel<GG, xor_rows64(GG)>), grid, dim3(kBlock), 0, stream, a, kc);
    });
}

// crc64_copy_iov_kernel<G>, as launch_copy.
int launch_copy_iov(const CopyIov64Args& a, int g, hipStream_t stream) {
    return launch_copying64(a.nmsg, g, stream, "crc64_copy_iov_kernel launch",
                            [&](auto G, dim3 grid, const LaneConsts64& kc) {
        hipLaunchKernelGGL(crc64_copy_iov_kernel<decltype(G)::value>, grid, dim3(kBlock), 0, stream, a, kc);
    });
}

// crc64_copy_iov_seg_kernel<G, DST> and the fold of its segment CRCs
// (DESIGN.md §4.6), both on `stream`: the grid as launch_copy_iov. Unlike
// the CRC-32C form, a second kernel folds: seed0, d_seeds and d_out go to it,
// not into the copy kernel's arguments.
int launch_copy_iov_seg(const CopyIovSeg64Args& a, bool dst_side, uint64_t seed0, const uint64_t* d_seeds,
                        uint64_t* d_out, int g, hipStream_t stream) {
    int copy_rc = 0;
    const int rc = launch_copying64(a.nmsg, g, stream, "crc64_seg_fold_kernel launch",
                                    [&](auto G, dim3 grid, const LaneConsts64& kc) {
        constexpr int GG = decltype(G)::value;
        if (dst_side)
            hipLaunchKernelGGL((crc64_copy_iov_seg_kernel<GG, true>), grid, dim3(kBlock), 0, stream, a, kc);
        else
            hipLaunchKernelGGL((crc64_copy_iov_seg_kernel<GG, false>), grid, dim3(kBlock), 0, stream, a, kc);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) {  // no fold after a copy kernel that was not enqueued
            copy_rc = hip_fail(e, "crc64_copy_iov_seg_kernel launch");
            return;
        }
        // inside the copy kernel's HeavyLaunch mark
        hipLaunchKernelGGL(crc64_seg_fold_kernel, dim3((a.nmsg + kSegFoldBlock / 64 - 1) / (kSegFoldBlock / 64)),
                           dim3(kSegFoldBlock), 0, stream, a, dst_side ? 1 : 0,
                           seed0, d_seeds, d_out, pow_table<Crc64>());
    });
    return copy_rc ? copy_rc : rc;
}

// The un-scan after a seg2 walk kernel, called from inside
// the walk's launch lambda: both launches sit in one HeavyLaunch mark, and no
// un-scan follows a walk kernel that was not enqueued.
template <typename W, typename A>
void launch_seg_unscan(const A& a, const char* walk_what, int* walk_rc, hipStream_t stream) {
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        *walk_rc = hip_fail(e, walk_what);
        return;
    }
    hipLaunchKernelGGL((seg_unscan_kernel<W, typename W::Pow>),
                       dim3((a.nmsg + kUnscanBlock / 64 - 1) / (kUnscanBlock / 64)), dim3(kUnscanBlock), 0, stream, a,
                       pow_table<W>());
}

// crc32c_copy_iov_seg2_kernel<G, U> and seg_unscan_kernel<Crc32c>, both on
// `stream`: the walk's grid as launch_copy_iov.
int launch_copy_iov_seg2(const CopyIovSeg2Args& a, int g, hipStream_t stream) {
    int walk_rc = 0;
    const int rc = launch_lanes<Crc32c>(a.nmsg, g, true, stream, "seg_unscan_kernel launch",
                                        [&](auto G, dim3 grid, const LaneConsts& kc) {
        constexpr int GG = decltype(G)::value;
        hipLaunchKernelGGL((crc32c_copy_iov_seg2_kernel<GG, default_rows(GG)>), grid, dim3(kBlock), 0, stream, a, kc);
        launch_seg_unscan<Crc32c>(a, "crc32c_copy_iov_seg2_kernel launch", &walk_rc, stream);
    });
    return walk_rc ? walk_rc : rc;
}

// crc64_copy_iov_seg2_kernel<G> and seg_unscan_kernel<Crc64>, as above.
int launch_copy_iov_seg2(const CopyIovSeg264Args& a, int g, hipStream_t stream) {
    int walk_rc = 0;
    const int rc = launch_copying64(a.nmsg, g, stream, "seg_unscan_kernel launch",
                                    [&](auto G, dim3 grid, const LaneConsts64& kc) {
        hipLaunchKernelGGL(crc64_copy_iov_seg2_kernel<decltype(G)::value>, grid, dim3(kBlock), 0, stream, a, kc);
        launch_seg_unscan<Crc64>(a, "crc64_copy_iov_seg2_kernel launch", &walk_rc, stream);
    });
    return walk_rc ? walk_rc : rc;
}

// The finish after a windowed walk kernel, as
// launch_seg_unscan: inside the walk's HeavyLaunch mark, and not after a walk
// kernel that was not enqueued.
template <typename W>
void launch_window_finish(const CopyIovWindowArgsT<typename W::T>& a, const char* walk_what, int* walk_rc,
                          hipStream_t stream) {
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        *walk_rc = hip_fail(e, walk_what);
        return;
    }
    hipLaunchKernelGGL((window_finish_kernel<W, typename W::Pow>),
                       dim3((a.nmsg + kUnscanBlock / 64 - 1) / (kUnscanBlock / 64)), dim3(kUnscanBlock), 0, stream, a,
                       pow_table<W>());
}

// crc32c_copy_iov_window_kernel<G, U> and window_finish_kernel<Crc32c>, both
// on `stream`: the walk's grid as launch_copy_iov.
int launch_copy_iov_window(const CopyIovWindowArgs& a, int g, hipStream_t stream) {
    int walk_rc = 0;
    const int rc = launch_lanes<Crc32c>(a.nmsg, g, true, stream, "window_finish_kernel launch",
                                        [&](auto G, dim3 grid, const LaneConsts& kc) {
        constexpr int GG = decltype(G)::value;
        hipLaunchKernelGGL((crc32c_copy_iov_window_kernel<GG, default_rows(GG)>), grid, dim3(kBlock), 0, stream, a,
                           kc);
        launch_window_finish<Crc32c>(a, "crc32c_copy_iov_window_kernel launch", &walk_rc, stream);
    });
    return walk_rc ? walk_rc : rc;
}

// crc64_copy_iov_window_kernel<G> and window_finish_kernel<Crc64>, as above.
int launch_copy_iov_window(const CopyIovWindow64Args& a, int g, hipStream_t stream) {
    int walk_rc = 0;
    const int rc = launch_copying64(a.nmsg, g, stream, "window_finish_kernel launch",
                                    [&](auto G, dim3 grid, const LaneConsts64& kc) {
        hipLaunchKernelGGL(crc64_copy_iov_window_kernel<decltype(G)::value>, grid, dim3(kBlock), 0, stream, a, kc);
        launch_window_finish<Crc64>(a, "crc64_copy_iov_window_kernel launch", &walk_rc, stream);
    });
    return walk_rc ? walk_rc : rc;
}

// Host-memory pipeline (photon_crc32c_host_batch_strided): per device, a copy
// stream and a compute stream, kNumStage device staging chunks. Chunk i is
// copied (H2D, 2-D so any host stride packs densely) while chunk i-1 is
// checksummed; events order reuse of a staging chunk after its kernel. The
// chunk arithmetic (kNumStage, kStageBytes, stage_plan) is host_chunks.h's.
// g_host_stage: the span of a staging chunk the pipeline fills, 0 = the whole
// allocation (photon_crc_set_host_stage_bytes; tests reach slot reuse with it).
std::atomic<uint64_t> g_host_stage{0};

struct HostPipe {
    std::mutex mu;  // one host-memory batch at a time per device; devices run concurrently
    bool ready = false;
    hipStream_t copy = nullptr, comp = nullptr;
    void* stage[kNumStage] = {};
    hipEvent_t copied[kNumStage] = {}, consumed[kNumStage] = {};
    void* d_out = nullptr;    // CRC words of the batch
    void* d_seeds = nullptr;
    uint64_t out_cap = 0;     // bytes
};

constexpr int kMaxDevices = 64;
HostPipe g_pipes[kMaxDevices];

// The device's pipeline, created on first use; the caller holds p.mu.
int pipe_init(HostPipe& p) {
    if (!p.ready) {
        hipError_t e;
        if ((e = hipStreamCreateWithFlags(&p.copy, hipStreamNonBlocking)) != hipSuccess) return hip_fail(e, "stream");
        if ((e = hipStreamCreateWithFlags(&p.comp, hipStreamNonBlocking)) != hipSuccess) return hip_fail(e, "stream");
        for (int i = 0; i < kNumStage; ++i) {
            if ((e = hipMalloc(&p.stage[i], kStageBytes)) != hipSuccess) return hip_fail(e, "hipMalloc(stage)");
            if ((e = hipEventCreateWithFlags(&p.copied[i], hipEventDisableTiming)) != hipSuccess)
                return hip_fail(e, "event");
            if ((e = hipEventCreateWithFlags(&p.consumed[i], hipEventDisableTiming)) != hipSuccess)
                return hip_fail(e, "event");
        }
        p.ready = true;
    }
    return 0;
}

// One long buffer (photon_crc32c_extend_device, photon_crc64ecma_extend_device):
// chunk 0 = the unaligned head up to the first 4 KiB boundary, then T-1
// aligned chunks of `chunk` bytes (a multiple of 1 KiB: whole rows),
// the last one cut at the end (crc32c_kernels.h "one long buffer"). Up to
// 256 KiB: at most 16 chunks of >= 4 KiB in one workgroup of 64-lane groups,
// the result written directly (latency). Above: chunks of >= 16 KiB,
// `rounds` chunks per lane group of a full grid (16 waves per CU; VERDICT r2:
// the piece batch used to fill half, or an eighth, of the chip), T equal to
// the grid's lane-group slots so every group gets the same number of chunks
// (chunk sizes were 4 KiB multiples before: up to one round of imbalance).
// Lane groups and rounds: tuning.h photon_crc_set_long_shape.
std::atomic<uint32_t> g_long_shape{0};  // lanes | rounds << 8; 0 = automatic

LongPlan long_plan(const void* data, uint64_t n, int cus, bool crc64) {
    return long_plan_for(data, n, cus, g_long_shape.load(std::memory_order_relaxed), 0, crc64);
}

// Run f() with this thread's stream-capture mode relaxed: the library's own
// one-time setup (hipMalloc, a copy on a private stream and its wait) is then
// legal even while some stream of the process -- possibly the caller's -- is
// being captured into a graph (global capture mode refuses such calls and
// invalidates the capture).
template <typename F>
hipError_t relaxed_capture(F f) {
    hipStreamCaptureMode m = hipStreamCaptureModeRelaxed;
    const hipError_t ex = hipThreadExchangeStreamCaptureMode(&m);
    const hipError_t e = f();
    if (ex == hipSuccess) (void)hipThreadExchangeStreamCaptureMode(&m);
    return e;
}

// The table-prologue images of the current device (crc32c_kernels.h
// load_tables, crc64_kernels.h load_tables64): table_image_kernel<G> /
// table_image64_kernel<G> write what build_tables<G> / build_tables64<G> leave
// in LDS, for every G, into one device buffer, and g_table_image /
// g_table_image64 point the kernels at it. Once per device, on its first call (current_device), on a
// private stream in relaxed capture mode. A failure leaves the slots null:
// the kernels then build their tables as before (same results).
void table_images_init() {
    (void)relaxed_capture([&] {
        constexpr uint64_t kB[10] = {lds_bytes_for<4>(),  lds_bytes_for<8>(),  lds_bytes_for<16>(), lds_bytes_for<32>(),
                                     lds_bytes_for<64>(), lds64_used<4>(),     lds64_used<8>(),     lds64_used<16>(),
                                     lds64_used<32>(),    lds64_used<64>()};
        uint64_t off[10], total = 0;
        for (int i = 0; i < 10; ++i) {
            off[i] = total;
            total += (kB[i] + 255) & ~255ull;
        }
        hipStream_t s = nullptr;
        char* base = nullptr;
        hipError_t r = hipStreamCreateWithFlags(&s, hipStreamNonBlocking);
        if (r == hipSuccess) r = hipMalloc(reinterpret_cast<void**>(&base), total);
        const uint32_t* img[5] = {};
        const uint32_t* img64[5] = {};
        for (int i = 0; i < 5; ++i) {
            img[i] = reinterpret_cast<const uint32_t*>(base + off[i]);
            img64[i] = reinterpret_cast<const uint32_t*>(base + off[5 + i]);
        }
        auto w = [&](int i) { return const_cast<uint32_t*>(img[i]); };
        auto w64 = [&](int i) { return const_cast<uint32_t*>(img64[i]); };
        if (r == hipSuccess) {
            hipLaunchKernelGGL(table_image_kernel<4>, dim3(1), dim3(kBlock), 0, s, lane_consts(4), w(0));
            hipLaunchKernelGGL(table_image_kernel<8>, dim3(1), dim3(kBlock), 0, s, lane_consts(8), w(1));
            hipLaunchKernelGGL(table_image_kernel<16>, dim3(1), dim3(kBlock), 0, s, lane_consts(16), w(2));
            hipLaunchKernelGGL(table_image_kernel<32>, dim3(1), dim3(kBlock), 0, s, lane_consts(32), w(3));
            hipLaunchKernelGGL(table_image_kernel<64>, dim3(1), dim3(kBlock), 0, s, lane_consts(64), w(4));
            hipLaunchKernelGGL(table_image64_kernel<4>, dim3(1), dim3(kBlock), 0, s, lane_consts64(4), w64(0));
            hipLaunchKernelGGL(table_image64_kernel<8>, dim3(1), dim3(kBlock), 0, s, lane_consts64(8), w64(1));
            hipLaunchKernelGGL(table_image64_kernel<16>, dim3(1), dim3(kBlock), 0, s, lane_consts64(16), w64(2));
            hipLaunchKernelGGL(table_image64_kernel<32>, dim3(1), dim3(kBlock), 0, s, lane_consts64(32), w64(3));
            hipLaunchKernelGGL(table_image64_kernel<64>, dim3(1), dim3(kBlock), 0, s, lane_consts64(64), w64(4));
            r = hipGetLastError();
        }
        if (r == hipSuccess) r = hipStreamSynchronize(s);  // the images are written before any kernel sees them
        bool published = false;  // once a slot may point into `base`, it is never freed
        if (r == hipSuccess) {
            published = true;
            r = hipMemcpyToSymbolAsync(HIP_SYMBOL(g_table_image), img, sizeof img, 0, hipMemcpyHostToDevice, s);
        }
        if (r == hipSuccess)
            r = hipMemcpyToSymbolAsync(HIP_SYMBOL(g_table_image64), img64, sizeof img64, 0, hipMemcpyHostToDevice, s);
        if (r == hipSuccess) r = hipStreamSynchronize(s);
        if (r != hipSuccess && base && !published) (void)hipFree(base);
        if (s) (void)hipStreamDestroy(s);
        return r;
    });
}

// A multi-workgroup launch captured into a HIP graph cannot use the stream's
// persistent reduce state (the graph would embed one ticket base and replay
// it). It gets a state of its own instead, owned by the graph being captured:
// zeroed, in reset mode (the last workgroup puts the ticket back to 0, so the
// graph replays any number of times), handed back to a per-device free list
// by a graph user object when the graph is destroyed. Replays of one graph
// run in order; two executable graphs instantiated from the SAME captured
// graph share its states and must not run at the same time (ADVICE r4:
// multi-workgroup captures used to be refused with -ENOTSUP).
constexpr uint64_t kStateBytes = 8 + 8 * kLongMaxGrid;
static_assert(8 * kTreeLine * (1 + kTreeGroups) <= kStateBytes, "long_reduce_tree words");
struct CapState {
    int dev;
    void* p;
};
std::mutex g_cap_mu;
std::vector<CapState*> g_cap_free;

void cap_state_release(void* arg) {  // graph user-object destructor: host bookkeeping only
    std::lock_guard<std::mutex> lk(g_cap_mu);
    g_cap_free.push_back(static_cast<CapState*>(arg));
}

int capture_state(hipStream_t st, void** out) {
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    unsigned long long id = 0;
    hipGraph_t graph = nullptr;
    hipError_t e = hipStreamGetCaptureInfo_v2(st, &cs, &id, &graph, nullptr, nullptr);
    if (e != hipSuccess) return hip_fail(e, "hipStreamGetCaptureInfo_v2");
    if (cs != hipStreamCaptureStatusActive || !graph) return fail(-ENOTSUP, "stream capture is not active");
    int dev = 0;
    if ((e = hipGetDevice(&dev)) != hipSuccess) return hip_fail(e, "hipGetDevice");
    CapState* c = nullptr;
    {
        std::lock_guard<std::mutex> lk(g_cap_mu);
        for (size_t i = 0; i < g_cap_free.size(); ++i)
            if (g_cap_free[i]->dev == dev) {
                c = g_cap_free[i];
                g_cap_free.erase(g_cap_free.begin() + (long)i);
                break;
            }
    }
    if (!c) {
        c = new CapState{dev, nullptr};
        e = relaxed_capture([&] {
            hipStream_t s = nullptr;
            hipError_t r = hipMalloc(&c->p, kStateBytes);
            if (r == hipSuccess) r = hipStreamCreateWithFlags(&s, hipStreamNonBlocking);
            if (r == hipSuccess) r = hipMemsetAsync(c->p, 0, kStateBytes, s);
            if (r == hipSuccess) r = hipStreamSynchronize(s);
            if (s) (void)hipStreamDestroy(s);
            return r;
        });
        if (e != hipSuccess) {
            if (c->p) (void)hipFree(c->p);
            delete c;
            return hip_fail(e, "capture reduce state");
        }
    }
    hipUserObject_t obj = nullptr;
    e = hipUserObjectCreate(&obj, c, cap_state_release, 1, hipUserObjectNoDestructorSync);
    if (e == hipSuccess) e = hipGraphRetainUserObject(graph, obj, 1, hipGraphUserObjectMove);
    if (e != hipSuccess) {
        if (obj) (void)hipUserObjectRelease(obj, 1);  // runs cap_state_release
        else cap_state_release(c);
        return hip_fail(e, "graph user object (capture reduce state)");
    }
    *out = c->p;
    return 0;
}

// hipStreamCaptureStatus of `st` (None when not capturing), or an error.
int capture_status(hipStream_t st, bool* capturing) {
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    const hipError_t e = hipStreamIsCapturing(st, &cs);
    if (e != hipSuccess) return hip_fail(e, "hipStreamIsCapturing");
    *capturing = cs != hipStreamCaptureStatusNone;
    return 0;
}

// long_reduce's state (ticket + slots) for a long-buffer launch on `st`: ONE
// buffer per (device, stream) -- per thread for hipStreamPerThread -- kept
// for the life of the process. Launches on one stream run in order, so the
// buffer needs no lease and no event: the scratch lease's hipEventRecord
// after every launch put a marker packet between back-to-back launches and
// cost 6 µs per 1 GiB call (scripts/ab_long.py probe+ev). Its 64-bit ticket
// is never reset (long_reduce): `base` counts the workgroups of every launch
// enqueued on the state so far, advanced under the state's lock in the same
// order as the launches are enqueued. If a destroyed stream's handle (or a
// recycled thread id's per-thread stream) comes back while the old stream's
// last launch still runs, the two launches may spoil each other's result,
// but the count stays exact for every later launch. A launch
// captured into a HIP graph uses a graph-owned state instead (capture_state:
// the graph would embed one `base` and replay it). lease != nullptr: a leased scratch buffer
// instead (more than 4096 streams seen), ticket 0 and put back to 0 by the
// kernel, to be returned with scratch_free.
struct LongState {
    void* p = nullptr;
    uint64_t base = 0;
    std::mutex mu;
};
std::mutex g_ls_mu;
std::map<std::tuple<int, uintptr_t, std::thread::id>, LongState*> g_long_state;

int long_state(hipStream_t st, LongState** out, void** lease) {
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return hip_fail(e, "hipGetDevice");
    const auto key = std::make_tuple(dev, reinterpret_cast<uintptr_t>(st),
                                     st == hipStreamPerThread ? std::this_thread::get_id() : std::thread::id());
    *out = nullptr;
    *lease = nullptr;
    {
        std::lock_guard<std::mutex> lk(g_ls_mu);
        auto it = g_long_state.find(key);
        if (it != g_long_state.end()) {
            *out = it->second;
            return 0;
        }
        if (g_long_state.size() >= 4096) return scratch_alloc(lease, kStateBytes, st, true);
    }
    auto* ls = new LongState;
    if ((e = hipMalloc(&ls->p, kStateBytes)) != hipSuccess) {
        delete ls;
        return hip_fail(e, "hipMalloc(long state)");
    }
    if ((e = hipMemsetAsync(ls->p, 0, kStateBytes, st)) != hipSuccess) {  // ordered before the launches on st
        (void)hipFree(ls->p);
        delete ls;
        return hip_fail(e, "hipMemset(long state)");
    }
    std::lock_guard<std::mutex> lk(g_ls_mu);
    auto ins = g_long_state.emplace(key, ls);
    if (!ins.second) {  // another thread registered this stream first
        (void)hipFree(ls->p);
        delete ls;
    }
    *out = ins.first->second;
    return 0;
}

// For an error message: the stream's reduce-state ticket on the device
// against the count the host expects after every enqueued launch.
std::string long_state_diag(hipStream_t st) {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return "";
    LongState* ls = nullptr;
    {
        std::lock_guard<std::mutex> lk(g_ls_mu);
        auto it = g_long_state.find(std::make_tuple(dev, reinterpret_cast<uintptr_t>(st), std::thread::id()));
        if (it == g_long_state.end()) return "; no reduce state";
        ls = it->second;
    }
    uint64_t ticket = 0;
    (void)hipStreamSynchronize(st);
    (void)hipMemcpy(&ticket, ls->p, 8, hipMemcpyDeviceToHost);
    std::lock_guard<std::mutex> lk(ls->mu);
    return "; reduce ticket " + std::to_string(ticket) + ", expected " + std::to_string(ls->base);
}

// Enqueue a long launch on its state: the state goes into the kernel's
// arguments `a` (acc, tbase, treset), then enqueue() launches the kernel with
// them; a persistent state's base advances by the grid only when the launch
// was enqueued, under its lock (launch order). kernel + what: the error text.
template <typename A, typename L>
int long_launch(hipStream_t st, uint64_t grid, const char* kernel, const char* what, A& a, L enqueue) {
    auto launch = [&](void* state, uint64_t base, uint32_t reset) {
        a.acc = static_cast<decltype(a.acc)>(state);
        a.tbase = base;
        a.treset = reset;
        enqueue();
        return hipGetLastError();
    };
    if (grid <= 1) {
        const hipError_t e = launch(nullptr, 0ull, 0u);
        return e == hipSuccess ? 0 : hip_fail(e, kernel, what);
    }
    bool capturing = false;
    if (int rc = capture_status(st, &capturing)) return rc;
    if (capturing) {  // a state owned by the graph, in reset mode
        void* cs = nullptr;
        if (int rc = capture_state(st, &cs)) return rc;
        const hipError_t e = launch(cs, 0ull, 1u);
        return e == hipSuccess ? 0 : hip_fail(e, kernel, what);
    }
    LongState* ls = nullptr;
    void* lease = nullptr;
    if (int rc = long_state(st, &ls, &lease)) return rc;
    if (lease) {
        const hipError_t e = launch(lease, 0ull, 1u);
        const int frc = scratch_free(lease, st);
        return e != hipSuccess ? hip_fail(e, kernel, what) : frc;
    }
    std::lock_guard<std::mutex> lk(ls->mu);
    const hipError_t e = launch(ls->p, ls->base, 0u);
    if (e != hipSuccess) return hip_fail(e, kernel, what);
    ls->base += grid;
    return 0;
}


// The small-buffer kernel's device image (crc32c_kernels.h "one small
// buffer"): its LDS tables and basis words, computed on the host with gf2.h
// and copied to each device once, on that device's first small call (a
// private non-blocking stream, so no other stream is synchronised).
template <typename W>
PerDevice<typename W::T*> g_img;

std::vector<uint32_t> small_image_host() {
    std::vector<uint32_t> img(kSmImage / 4, 0u);
    auto nibbles = [&](uint32_t off, uint32_t k) {  // (v << 4t) * k, t < 8, v < 16, at byte offset off
        for (uint32_t t = 0; t < 8; ++t)
            for (uint32_t v = 0; v < 16; ++v) img[off / 4 + t * 16 + v] = mulmod(v << (4 * t), k);
    };
    for (uint32_t j = 1; j <= 3; ++j) nibbles(kSmD + (j - 1) * kNib, xpow(32ull * j));  // x^(32 j)
    nibbles(kSmS, xpow(8ull * 16ull * kSmallLanes));        // one row of the small layout's V blocks
    for (uint32_t dl = 0; dl < 8; ++dl) nibbles(kSmA + dl * kNib, xpow(32ull + 128ull * dl));
    for (uint32_t dh = 1; dh < 8; ++dh) nibbles(kSmB + (dh - 1) * kNib, xpow(1024ull * dh));
    nibbles(kSmS2, xpow(8ull * 16ull * kMidLanes));         // one row of the mid layout's
    const uint32_t step = xpow(8192ull);                      // one wave of 64 blocks
    uint32_t k = xpow(0);
    for (uint32_t d = 0; d < 4 * kMidWg; ++d, k = mulmod(k, step))  // d waves after this one
        mul_basis(k, &img[kSmWave / 4 + d * 32]);
    for (uint32_t k = 0; k < 32; ++k) mul_basis(xpow_inv(8ull * k), &img[kSmTail / 4 + k * 32]);
    return img;
}



// Copy `bytes` of host words to a new device buffer of the current device.
template <typename T>
int upload_image(const std::vector<T>& host, uint64_t bytes, T** out, const char* what) {
    void* d = nullptr;
    const hipError_t e = relaxed_capture([&] {  // legal during a caller's graph capture
        hipStream_t s = nullptr;
        hipError_t r = hipMalloc(&d, bytes);
        if (r == hipSuccess) r = hipStreamCreateWithFlags(&s, hipStreamNonBlocking);
        if (r == hipSuccess) r = hipMemcpyAsync(d, host.data(), bytes, hipMemcpyHostToDevice, s);
        if (r == hipSuccess) r = hipStreamSynchronize(s);
        if (s) (void)hipStreamDestroy(s);
        return r;
    });
    if (e != hipSuccess) {
        if (d) (void)hipFree(d);
        return hip_fail(e, what);
    }
    *out = static_cast<T*>(d);
    return 0;
}

// The CRC-64 small kernel's image (crc64_kernels.h crc64_small_kernel), as
// small_image_host: nibble tables [position][value] of x^64, x^(128 V), x^(64 +
// 128 dl), x^(1024 dh), then the wave and tail basis words.
std::vector<uint64_t> small64_image_host() {
    std::vector<uint64_t> img(kSm64Image / 8, 0ull);
    auto nibbles = [&](uint32_t off, uint64_t k) {  // (v << 4t) * k, t < 16, v < 16
        for (uint32_t t = 0; t < 16; ++t)
            for (uint32_t v = 0; v < 16; ++v) img[off / 8 + t * 16 + v] = mulmod64((uint64_t)v << (4 * t), k);
    };
    nibbles(kSm64D, xpow64(64));
    nibbles(kSm64S, xpow64(8ull * 16ull * kSmallLanes));
    for (uint32_t dl = 0; dl < 8; ++dl) nibbles(kSm64A + dl * kNib64, xpow64(64ull + 128ull * dl));
    for (uint32_t dh = 1; dh < 8; ++dh) nibbles(kSm64B + (dh - 1) * kNib64, xpow64(1024ull * dh));
    nibbles(kSm64S2, xpow64(8ull * 16ull * kMidLanes));
    const uint64_t step = xpow64(8192ull);
    uint64_t k = xpow64(0);
    for (uint32_t d = 0; d < 4 * kMidWg; ++d, k = mulmod64(k, step))  // d waves after this one
        for (int i = 0; i < 64; ++i) img[kSm64Wave / 8 + d * 64 + i] = mulmod64(1ull << i, k);
    for (uint32_t k = 0; k < 32; ++k) {
        const uint64_t kk = xpow64_inv(8ull * k);
        for (int i = 0; i < 64; ++i) img[kSm64Tail / 8 + k * 64 + i] = mulmod64(1ull << i, kk);
    }
    return img;
}

// The image of device `dev` (the caller's current device: multi-device paths
// set it first, multi_device.h).
template <typename W>
int small_image(int dev, const typename W::T** out) {
    typename W::T* p = nullptr;
    const int rc = g_img<W>.get(dev, &p, [](int, typename W::T*& slot) {
        static const std::vector<typename W::T> host = W::image_host();
        return upload_image(host, W::kImageBytes, &slot, W::kImageName);
    });
    *out = p;
    return rc;
}

// The small kernel's geometry for [p, p + n), or false when the block span
// exceeds max_blocks (kSmallBlocks: the long kernel's case; the service takes
// up to kSvcMaxBlocks). *grid = the workgroups that
// hold data (the last ones of the layout).
template <typename W>
bool small_args(const void* p, uint64_t n, typename W::T seed, typename W::Small* a, uint32_t* grid,
                uint64_t max_blocks = kSmallBlocks) {
    const uintptr_t d = reinterpret_cast<uintptr_t>(p);
    const uint64_t s0 = d & 15u, eoff = s0 + n;
    const uint64_t cover = eoff > s0 + W::kSeedBytes ? eoff : s0 + W::kSeedBytes;  // the seed's bytes lie inside the grid
    const uint64_t nb = (cover + 15) >> 4;
    if (nb > max_blocks) return false;
    a->a0 = reinterpret_cast<const uint8_t*>(d - s0);
    a->nb = (uint32_t)nb;
    a->s0 = (uint32_t)s0;
    a->eoff = (uint32_t)eoff;
    a->k = (uint32_t)(16 * nb - eoff);
    W::put_seed(a, seed);
    *grid = nb > kSmallLanes ? kSmallWg : (uint32_t)((nb + 255) / 256);
    a->wg0 = kSmallWg - *grid;
    return true;
}

// The mid layout (crc32c_kernels.h kMidWg): spans over kSmallBlocks up to
// kMidBlocks (16 MiB, both CRCs) while
// photon_crc_set_mid_kernel is on, else false (the long kernel's case).
std::atomic<int> g_mid_kernel{1};

template <typename W>
bool mid_args(const void* p, uint64_t n, typename W::T seed, typename W::Small* a, uint32_t* grid) {
    if (!g_mid_kernel.load(std::memory_order_relaxed) || !small_args<W>(p, n, seed, a, grid, W::kMidBlocks))
        return false;
    *grid = a->nb > kMidLanes ? kMidWg : (a->nb + 255) / 256;
    a->wg0 = kMidWg - *grid;
    return true;
}

// photon_crc_test_small_plan for one CRC width: the launch paths' own
// small_args / mid_args (extend_device, dispatch_crc), nothing launched.
template <typename W>
int test_small_plan(const void* p, uint64_t n, uint64_t* out, int nout) {
    typename W::Small sa{};
    uint32_t grid = 0, v = 0, layout = 2;
    const bool svc = small_args<W>(p, n, 0, &sa, &grid, kSvcMaxBlocks);  // as dispatch_crc asks
    sa = typename W::Small{};
    if (small_args<W>(p, n, 0, &sa, &grid)) {
        layout = 0;
        v = kSmallLanes;
    } else if (mid_args<W>(p, n, 0, &sa, &grid)) {
        layout = 1;
        v = kMidLanes;
    } else {  // the long kernel's case: no block grid
        sa = typename W::Small{};
        grid = 0;
    }
    const uint64_t rows = v ? (sa.nb + v - 1) / v : 0;  // as small_wave_value / small_load count them
    const uint64_t w[] = {layout, sa.nb, sa.s0, sa.eoff, sa.k, rows, grid, sa.wg0, svc,
                          kSmallLanes, kSmallWg, kMidLanes, kMidWg, kSmallBlocks, W::kMidBlocks,
                          kSmallRows, W::kMidRows, kSvcMaxBlocks, W::kSeedBytes};
    constexpr int kn = (int)(sizeof w / sizeof w[0]);
    if (nout < kn) return fail(-EINVAL, "short output");
    memcpy(out, w, sizeof w);
    return kn;
}

// The long kernel for photon_crc32c_extend_device / photon_crc64ecma_extend_device
// (and, with a tag, for a routed call whose result lands tagged in pinned memory).
template <typename W>
int extend_device_long(const void* d_data, uint64_t nbytes, typename W::T seed, typename W::T* d_out, hipStream_t st,
                       int cus, uint32_t tag) {
    const LongPlan lp = long_plan(d_data, nbytes, cus, W::kCrc64);
    const LongPowers& pw = long_powers(lp, W::kCrc64);
    typename W::Long a{};
    W::long_args(&a, lp, pw, d_data, seed, d_out);
    a.out_tag = tag;
    HeavyLaunch heavy(st);
    return long_launch(st, lp.grid, W::kKernel, "_long_kernel launch", a, [&] {
        if (lp.lanes == 32)
            hipLaunchKernelGGL(W::template long_kernel<32>(), dim3(lp.grid), dim3(kBlock), 0, st, a, W::lanes(32));
        else
            hipLaunchKernelGGL(W::template long_kernel<64>(), dim3(lp.grid), dim3(kBlock), 0, st, a, W::lanes(64));
    });
}

// A span over the small kernel's: the mid layout up to 16 MiB, else the long
// kernel (tag: as extend_device_long).
template <typename W>
int extend_device_big(int dev, const void* d_data, uint64_t nbytes, typename W::T seed, typename W::T* d_out,
                      hipStream_t st, int cus, uint32_t tag) {
    typename W::Small sa{};
    uint32_t grid = 0;
    if (!mid_args<W>(d_data, nbytes, seed, &sa, &grid))
        return extend_device_long<W>(d_data, nbytes, seed, d_out, st, cus, tag);
    if (int rc = small_image<W>(dev, &sa.image)) return rc;
    sa.out = d_out;
    sa.tag = tag;  // slots unset: the tag goes to long_reduce's result word(s)
    return long_launch(st, grid, W::kKernel, "_small_kernel (mid) launch", sa, [&] {
        hipLaunchKernelGGL((W::template small_kernel<kMidLanes, W::kMidRows>()), dim3(grid), dim3(256), 0, st, sa);
    });
}

// photon_crc32c_extend_device / photon_crc64ecma_extend_device.
template <typename W>
int extend_device(const void* d_data, uint64_t nbytes, typename W::T seed, typename W::T* d_out, void* stream) {
    if (!d_out || (!d_data && nbytes)) return fail(-EINVAL, "null buffer or output");
    hipStream_t st = static_cast<hipStream_t>(stream);
    int cus = 0;
    int dev = current_device(&cus);
    if (dev < 0) return dev;
    typename W::Small sa{};
    uint32_t sgrid = 0;
    if (small_args<W>(d_data, nbytes, seed, &sa, &sgrid)) {  // <= 256 KiB: the latency path
        if (int rc = small_image<W>(dev, &sa.image)) return rc;
        sa.out = d_out;
        return long_launch(st, sgrid, W::kKernel, "_small_kernel launch", sa, [&] {
            hipLaunchKernelGGL((W::template small_kernel<kSmallLanes, kSmallRows>()), dim3(sgrid), dim3(256), 0, st,
                               sa);
        });
    }
    return extend_device_big<W>(dev, d_data, nbytes, seed, d_out, st, cus, 0);
}

// photon_crc32c_copy_extend_device / photon_crc64ecma_copy_extend_device:
// extend_device_long's plan, powers and state with the copying kernel. Every
// size comes here (the plan's `small` branch serves spans up to 256 KiB).
template <typename W>
int copy_extend_device(const void* src, void* d_dst, uint64_t nbytes, typename W::T seed, typename W::T* d_out,
                       void* stream) {
    if (!d_out || ((!src || !d_dst) && nbytes)) return fail(-EINVAL, "null source, destination or output");
    hipStream_t st = static_cast<hipStream_t>(stream);
    int cus = 0;
    int dev = current_device(&cus);
    if (dev < 0) return dev;
    const LongPlan lp = long_plan(src, nbytes, cus, W::kCrc64);
    const LongPowers& pw = long_powers(lp, W::kCrc64);
    typename W::CopyLong a{};
    W::long_args(&a, lp, pw, src, seed, d_out);
    a.dst = static_cast<uint8_t*>(d_dst);
    HeavyLaunch heavy(st);
    return long_launch(st, lp.grid, W::kKernel, "_copy_long_kernel launch", a, [&] {
        if (lp.lanes == 32)
            hipLaunchKernelGGL(W::template copy_long_kernel<32>(), dim3(lp.grid), dim3(kBlock), 0, st, a,
                               W::lanes(32));
        else
            hipLaunchKernelGGL(W::template copy_long_kernel<64>(), dim3(lp.grid), dim3(kBlock), 0, st, a,
                               W::lanes(64));
    });
}

// photon_crc32c_batch_strided / photon_crc64ecma_batch_strided.
template <typename W>
int batch_strided(const void* d_base, uint64_t stride, uint64_t nbytes, uint64_t count, typename W::T seed0,
                  const typename W::T* d_seeds, typename W::T* d_out, void* stream) {
    if (count && (!d_out || (!d_base && nbytes))) return fail(-EINVAL, "null buffer or output");
    typename W::Batch a{};
    a.base = static_cast<const uint8_t*>(d_base);
    a.stride = stride;
    a.nbytes = nbytes;
    a.count = count;
    a.seeds = d_seeds;
    a.out = d_out;
    a.seed0 = seed0;
    if (W::kShiftInit && !d_seeds && !(reinterpret_cast<uintptr_t>(d_base) & 15) && !(stride & 15) && nbytes >= 64) {
        a.shift_init = 1;
        a.init_shift = W::shift_init(seed0, nbytes);
    }
    return launch_batch(a, nbytes, static_cast<hipStream_t>(stream));
}

// photon_crc32c_batch_iov / photon_crc64ecma_batch_iov.
template <typename W>
int batch_iov(const photon_crc_iovec* d_iov, uint64_t count, typename W::T seed0, const typename W::T* d_seeds,
              typename W::T* d_out, void* stream) {
    if (count && (!d_iov || !d_out)) return fail(-EINVAL, "null descriptor array or output");
    typename W::Batch a{};
    a.iov = d_iov;
    a.count = count;
    a.seeds = d_seeds;
    a.out = d_out;
    a.seed0 = seed0;
    // Descriptors live on the device; lengths are unknown to the host, so the
    // lane-group size is the generic one unless overridden.
    return launch_batch(a, 65536, static_cast<hipStream_t>(stream));
}

// Copy + CRC in one pass (crc32c_gpu.h; DESIGN.md "Copy + CRC", §4.4):
// photon_crc32c_copy_batch_strided / photon_crc64ecma_copy_batch_strided.
template <typename W>
int copy_batch_strided(const void* src_base, uint64_t src_stride, void* d_dst_base, uint64_t dst_stride,
                       uint64_t nbytes, uint64_t count, typename W::T seed0, const typename W::T* d_seeds,
                       typename W::T* d_out, void* stream) {
    if (!count) return 0;
    if (!d_out || ((!src_base || !d_dst_base) && nbytes)) return fail(-EINVAL, "null source, destination or output");
    typename W::CopyBatch a{};
    a.base = static_cast<const uint8_t*>(src_base);
    a.stride = src_stride;
    a.nbytes = nbytes;
    a.count = count;
    a.seeds = d_seeds;
    a.out = d_out;
    a.seed0 = seed0;
    a.dst_base = static_cast<uint8_t*>(d_dst_base);
    a.dst_stride = dst_stride;
    if (W::kShiftInit && !d_seeds && !(reinterpret_cast<uintptr_t>(src_base) & 15) && !(src_stride & 15) &&
        nbytes >= 64) {
        a.shift_init = 1;
        a.init_shift = W::shift_init(seed0, nbytes);
    }
    return launch_copy(a, count, W::copy_lanes(nbytes), static_cast<hipStream_t>(stream));
}

// photon_crc32c_copy_batch_iov / photon_crc64ecma_copy_batch_iov.
template <typename W>
int copy_batch_iov(const photon_crc_iovec* d_src, void* const* d_dst, uint64_t count, typename W::T seed0,
                   const typename W::T* d_seeds, typename W::T* d_out, void* stream) {
    if (!count) return 0;
    if (!d_src || !d_dst || !d_out) return fail(-EINVAL, "null descriptor array, destination array or output");
    typename W::CopyBatch a{};
    a.iov = d_src;
    a.count = count;
    a.seeds = d_seeds;
    a.out = d_out;
    a.seed0 = seed0;
    a.dst = d_dst;
    return launch_copy(a, count, W::copy_lanes(65536), static_cast<hipStream_t>(stream));
}

// photon_crc32c_copy_msg_iov_n / photon_crc64ecma_copy_msg_iov_n.
template <typename W>
int copy_msg_iov_n(const photon_crc_iovec* d_src, const uint64_t* d_src_start, uint64_t nsrc,
                   const photon_crc_iovec* d_dst, const uint64_t* d_dst_start, uint64_t ndst, uint64_t nmsg,
                   const uint64_t* d_size, typename W::T seed0, const typename W::T* d_seeds, typename W::T* d_out,
                   uint64_t* d_copied, void* stream) {
    if (!nmsg) return 0;
    if (!d_src_start || !d_dst_start || !d_out || (!d_src && nsrc) || (!d_dst && ndst))
        return fail(-EINVAL, "null argument");
    // Lane groups as the gather takes (choose_lanes(8192)).
    typename W::CopyIov a{};
    a.src = d_src;
    a.src_start = d_src_start;
    a.dst = d_dst;
    a.dst_start = d_dst_start;
    a.nmsg = nmsg;
    a.size = d_size;
    a.seeds = d_seeds;
    a.out = d_out;
    a.copied = d_copied;
    a.seed0 = seed0;
    return launch_copy_iov(a, choose_lanes(8192), static_cast<hipStream_t>(stream));
}

// photon_crc32c_copy_msg_iov_seg2_n / photon_crc64ecma_copy_msg_iov_seg2_n.
template <typename W>
int copy_msg_iov_seg2_n(const photon_crc_iovec* d_src, const uint64_t* d_src_start, uint64_t nsrc,
                        const photon_crc_iovec* d_dst, const uint64_t* d_dst_start, uint64_t ndst, uint64_t nmsg,
                        const uint64_t* d_size, typename W::T seed0, const typename W::T* d_seeds,
                        typename W::T* d_src_seg_out, typename W::T* d_dst_seg_out, typename W::T* d_out,
                        uint64_t* d_copied, void* stream) {
    if (!nmsg) return 0;
    if (!d_src_start || !d_dst_start || !d_out || !d_src_seg_out || !d_dst_seg_out || (!d_src && nsrc) ||
        (!d_dst && ndst))
        return fail(-EINVAL, "null argument");
    CopyIovSeg2ArgsT<typename W::T> a{};
    a.src = d_src;
    a.src_start = d_src_start;
    a.dst = d_dst;
    a.dst_start = d_dst_start;
    a.nmsg = nmsg;
    a.size = d_size;
    a.seeds = d_seeds;
    a.src_seg = d_src_seg_out;
    a.dst_seg = d_dst_seg_out;
    a.out = d_out;
    a.copied = d_copied;
    a.seed0 = seed0;
    return launch_copy_iov_seg2(a, choose_lanes(8192), static_cast<hipStream_t>(stream));
}

// photon_crc32c_copy_msg_iov_window_n / photon_crc64ecma_copy_msg_iov_window_n.
template <typename W>
int copy_msg_iov_window_n(const photon_crc_iovec* d_src, const uint64_t* d_src_start, uint64_t nsrc,
                          const photon_crc_iovec* d_dst, const uint64_t* d_dst_start, uint64_t ndst, uint64_t nmsg,
                          const uint64_t* d_skip, const uint64_t* d_size, typename W::T seed0,
                          const typename W::T* d_seeds, typename W::T* d_src_seg_out, typename W::T* d_out,
                          uint64_t* d_copied, void* d_work, void* stream) {
    if (!nmsg) return 0;
    if (!d_src_start || !d_dst_start || !d_out || !d_src_seg_out || !d_work || (!d_src && nsrc) || (!d_dst && ndst))
        return fail(-EINVAL, "null argument");
    CopyIovWindowArgsT<typename W::T> a{};
    a.src = d_src;
    a.src_start = d_src_start;
    a.dst = d_dst;
    a.dst_start = d_dst_start;
    a.nmsg = nmsg;
    a.skip = d_skip;
    a.size = d_size;
    a.seeds = d_seeds;
    a.src_seg = d_src_seg_out;
    a.out = d_out;
    a.copied = d_copied;
    a.work = static_cast<uint64_t*>(d_work);
    a.seed0 = seed0;
    return launch_copy_iov_window(a, choose_lanes(8192), static_cast<hipStream_t>(stream));
}

// photon_crc32c_combine_batch / photon_crc64ecma_combine_batch.
template <typename W>
int combine_batch(const typename W::T* d_crc1, const typename W::T* d_crc2, const uint32_t* d_len2, uint64_t count,
                  typename W::T* d_out, void* stream) {
    if (!count) return 0;
    if (!d_crc1 || !d_crc2 || !d_len2 || !d_out) return fail(-EINVAL, "null argument");
    int cus = 0;
    int dev = current_device(&cus);
    if (dev < 0) return dev;
    hipLaunchKernelGGL(W::kCombineKernel, dim3((count + 255) / 256), dim3(256), 0, static_cast<hipStream_t>(stream),
                       d_crc1, d_crc2, d_len2, count, d_out, pow_table<W>());
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : hip_fail(e, W::kKernel, "_combine_kernel launch");
}

// photon_crc32c_trim_batch / photon_crc64ecma_trim_batch (C: photon_crc_component,
// photon_crc64_component).
template <typename W, typename C>
int trim_batch(const C* d_all, const C* d_prefix, const C* d_suffix, uint64_t count, typename W::T* d_out,
               uint32_t* d_nerr, void* stream) {
    if (!count) return 0;
    if (!d_all || !d_prefix || !d_suffix || !d_out) return fail(-EINVAL, "null argument");
    int cus = 0;
    int dev = current_device(&cus);
    if (dev < 0) return dev;
    hipLaunchKernelGGL(W::kTrimKernel, dim3((count + 255) / 256), dim3(256), 0, static_cast<hipStream_t>(stream),
                       d_all, d_prefix, d_suffix, count, d_out, d_nerr, pow_table<W>(), rshift_table<W>());
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : hip_fail(e, W::kKernel, "_trim_kernel launch");
}

// photon_crc32c_series_device / photon_crc64ecma_series_device: parts below
// W::kSeriesMinPart bytes give 0 and are not read.
template <typename W>
int series_device(const void* d_buffer, uint32_t part_size, uint32_t n_parts, typename W::T* d_crc_parts,
                  void* stream) {
    if (!n_parts) return 0;
    if (!d_crc_parts || (!d_buffer && part_size)) return fail(-EINVAL, "null buffer or output");
    if (part_size < W::kSeriesMinPart) {
        int cus = 0;
        int dev = current_device(&cus);
        if (dev < 0) return dev;
        const hipError_t e =
            hipMemsetAsync(d_crc_parts, 0, sizeof(typename W::T) * n_parts, static_cast<hipStream_t>(stream));
        return e == hipSuccess ? 0 : hip_fail(e, "hipMemsetAsync");
    }
    return batch_strided<W>(d_buffer, part_size, part_size, n_parts, 0, nullptr, d_crc_parts, stream);
}

// photon_crc32c_combine_series_device / photon_crc64ecma_combine_series_device.
template <typename W>
int combine_series_device(const typename W::T* d_crc, uint32_t part_size, uint32_t n_parts, typename W::T* d_result,
                          void* stream) {
    if (!d_result || (!d_crc && n_parts)) return fail(-EINVAL, "null argument");
    int cus = 0;
    int dev = current_device(&cus);
    if (dev < 0) return dev;
    hipStream_t st = static_cast<hipStream_t>(stream);
    hipError_t e = hipMemsetAsync(d_result, 0, sizeof(typename W::T), st);
    if (e != hipSuccess) return hip_fail(e, "hipMemsetAsync");
    if (!n_parts) return 0;
    if (!W::combine_series_of_empty(d_crc, part_size, n_parts, d_result, st)) {
        const uint64_t threads = ((uint64_t)n_parts + kSeriesChunk - 1) / kSeriesChunk;
        hipLaunchKernelGGL(W::kCombineSeriesKernel, dim3((threads + 255) / 256), dim3(256), 0, st, d_crc,
                           (uint64_t)n_parts, d_result, part_pow_table<W>(part_size));
    }
    e = hipGetLastError();
    return e == hipSuccess ? 0 : hip_fail(e, W::kCombineSeriesLaunch);
}

// Workgroup size of the fold_parts kernels by parts per object (the host
// knows the average only): a wave for up to 64, 256 threads up to 1,024,
// 1,024 threads above.
uint32_t fold_parts_block_size(uint64_t nobj, uint64_t nparts) {
    const uint64_t avg = nparts / nobj;
    return avg <= 64 ? 64u : avg <= 1024 ? 256u : (uint32_t)kFoldMaxBlock;
}

// photon_crc32c_fold_parts_n / photon_crc64ecma_fold_parts_n.
template <typename W>
int fold_parts_n(const typename W::T* d_crc, const uint64_t* d_len, const uint64_t* d_obj_start, uint64_t nobj,
                 uint64_t nparts, typename W::T seed0, const typename W::T* d_seeds, typename W::T* d_out,
                 uint64_t* d_total, void* stream) {
    if (!nobj) return 0;
    if (!d_out) return fail(-EINVAL, "null output");
    if ((!d_crc || !d_len) && nparts) return fail(-EINVAL, "null part CRCs or lengths");
    if (!d_obj_start && nobj != 1) return fail(-EINVAL, "a null d_obj_start means one object: nobj must be 1");
    int cus = 0;
    int dev = current_device(&cus);
    if (dev < 0) return dev;
    const uint32_t grid = nobj < kFoldMaxGrid ? (uint32_t)nobj : kFoldMaxGrid;
    hipLaunchKernelGGL(W::kFoldPartsKernel, dim3(grid), dim3(fold_parts_block_size(nobj, nparts)), 0,
                       static_cast<hipStream_t>(stream), d_crc, d_len, d_obj_start, nobj, nparts, seed0, d_seeds,
                       d_out, d_total, pow_table<W>());
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : hip_fail(e, W::kKernel, "_fold_parts_kernel launch");
}

// Overwrite + CRC delta (crc32c_gpu.h):
// photon_crc32c_overwrite_batch_strided / photon_crc64ecma_overwrite_batch_strided.
// Lanes as the copy calls take them (W::copy_lanes).
template <typename W>
int overwrite_batch_strided(const void* src_base, uint64_t src_stride, void* d_dst_base, uint64_t dst_stride,
                            uint64_t nbytes, uint64_t count, typename W::T* d_delta, void* stream) {
    if (!count) return 0;
    if (!d_delta || ((!src_base || !d_dst_base) && nbytes)) return fail(-EINVAL, "null source, destination or delta output");
    OverwriteArgs<typename W::T> a{};
    a.base = static_cast<const uint8_t*>(src_base);
    a.stride = src_stride;
    a.nbytes = nbytes;
    a.count = count;
    a.dst_base = static_cast<uint8_t*>(d_dst_base);
    a.dst_stride = dst_stride;
    a.out = d_delta;
    return launch_overwrite(a, W::copy_lanes(nbytes), static_cast<hipStream_t>(stream));
}

// photon_crc32c_overwrite_batch_iov / photon_crc64ecma_overwrite_batch_iov.
template <typename W>
int overwrite_batch_iov(const photon_crc_iovec* d_src, void* const* d_dst, uint64_t count, typename W::T* d_delta,
                        void* stream) {
    if (!count) return 0;
    if (!d_src || !d_dst || !d_delta) return fail(-EINVAL, "null descriptor array, destination array or delta output");
    OverwriteArgs<typename W::T> a{};
    a.iov = d_src;
    a.count = count;
    a.dst = d_dst;
    a.out = d_delta;
    return launch_overwrite(a, W::copy_lanes(65536), static_cast<hipStream_t>(stream));
}

// photon_crc32c_patch_n / photon_crc64ecma_patch_n: one launch, the workgroup
// size by writes per target as the fold picks its own by parts per object.
template <typename W>
int patch_n(const typename W::T* d_delta, const uint64_t* d_tail, uint64_t nwrites, const uint64_t* d_tgt_start,
            uint64_t ntgt, const typename W::T* d_crc_in, typename W::T* d_crc_out, void* stream) {
    if (!ntgt) return 0;
    if (!d_crc_in || !d_crc_out) return fail(-EINVAL, "null CRC input or output");
    if ((!d_delta || !d_tail) && nwrites) return fail(-EINVAL, "null deltas or tails");
    if (!d_tgt_start && ntgt != nwrites)
        return fail(-EINVAL, "a null d_tgt_start means write i patches word i: ntgt must equal nwrites");
    int cus = 0;
    int dev = current_device(&cus);
    if (dev < 0) return dev;
    const uint32_t grid = ntgt < kFoldMaxGrid ? (uint32_t)ntgt : kFoldMaxGrid;
    hipLaunchKernelGGL((patch_kernel<W, typename W::Pow>), dim3(grid), dim3(fold_parts_block_size(ntgt, nwrites)), 0,
                       static_cast<hipStream_t>(stream), d_delta, d_tail, nwrites, d_tgt_start, ntgt, d_crc_in,
                       d_crc_out, pow_table<W>());
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : hip_fail(e, W::kKernel, "_patch_kernel launch");
}

// Stripe parity + CRC (crc32c_gpu.h):
// photon_crc32c_xor_batch_strided / photon_crc64ecma_xor_batch_strided.
// Lanes as the copy calls take them (W::copy_lanes).
template <typename W>
int xor_batch_strided(const void* src_base, uint64_t stripe_stride, uint64_t block_stride, uint32_t k,
                      void* d_dst_base, uint64_t dst_stride, uint64_t nbytes, uint64_t count, typename W::T seed0,
                      const typename W::T* d_seeds, typename W::T* d_out, void* stream) {
    if (!count) return 0;
    if (k < 1 || k > kXorMaxSources) return fail(-EINVAL, "a stripe has 1 to 64 sources");
    if (!d_out || ((!src_base || !d_dst_base) && nbytes)) return fail(-EINVAL, "null source, parity or CRC output");
    XorArgs<typename W::T> a{};
    a.base = static_cast<const uint8_t*>(src_base);
    a.stripe_stride = stripe_stride;
    a.block_stride = block_stride;
    a.nbytes = nbytes;
    a.dst_base = static_cast<uint8_t*>(d_dst_base);
    a.dst_stride = dst_stride;
    a.k = k;
    a.count = count;
    a.seed0 = seed0;
    a.seeds = d_seeds;
    a.out = d_out;
    return launch_xor(a, W::copy_lanes(nbytes), static_cast<hipStream_t>(stream));
}

// photon_crc32c_xor_batch_ptr / photon_crc64ecma_xor_batch_ptr.
template <typename W>
int xor_batch_ptr(const void* const* d_src, uint32_t k, const photon_crc_iovec* d_dst, uint64_t count,
                  typename W::T seed0, const typename W::T* d_seeds, typename W::T* d_out, void* stream) {
    if (!count) return 0;
    if (k < 1 || k > kXorMaxSources) return fail(-EINVAL, "a stripe has 1 to 64 sources");
    if (!d_src || !d_dst || !d_out) return fail(-EINVAL, "null source pointer array, parity descriptors or CRC output");
    XorArgs<typename W::T> a{};
    a.src = d_src;
    a.dstv = d_dst;
    a.k = k;
    a.count = count;
    a.seed0 = seed0;
    a.seeds = d_seeds;
    a.out = d_out;
    return launch_xor(a, W::copy_lanes(65536), static_cast<hipStream_t>(stream));
}

// The inversion of the register on the way in and out (xor_expect.h).
template <typename W>
constexpr typename W::T xor_expect_inv() {
    return sizeof(typename W::T) == 8 ? ~(typename W::T)0 : 0;
}

bool xor_expect_args_ok(const void* crc, uint64_t ncrc, const uint64_t* grp_start, uint32_t k, const void* want) {
    if (!want) return false;
    if (!crc && ncrc) return false;
    return grp_start || (k >= 1 && k <= kXorMaxSources);
}
constexpr const char* kXorExpectArgs =
    "null words with ncrc > 0, null output, or a null d_grp_start with k outside 1 to 64";

// photon_crc32c_xor_expect_n / photon_crc64ecma_xor_expect_n: one launch, a
// thread per stripe.
template <typename W>
int xor_expect_n(const typename W::T* d_crc, uint64_t ncrc, const uint64_t* d_grp_start, uint32_t k,
                 const uint64_t* d_len, uint64_t nbytes, uint64_t count, typename W::T seed, typename W::T* d_want,
                 void* stream) {
    if (!count) return 0;
    if (!xor_expect_args_ok(d_crc, ncrc, d_grp_start, k, d_want)) return fail(-EINVAL, kXorExpectArgs);
    int cus = 0;
    int dev = current_device(&cus);
    if (dev < 0) return dev;
    const uint64_t blocks = (count + kXorExpectBlock - 1) / kXorExpectBlock;
    const uint32_t grid = blocks < kFoldMaxGrid ? (uint32_t)blocks : kFoldMaxGrid;
    hipLaunchKernelGGL((xor_expect_kernel<W, typename W::Pow>), dim3(grid), dim3(kXorExpectBlock), 0,
                       static_cast<hipStream_t>(stream), d_crc, ncrc, d_grp_start, k, d_len, nbytes, count, seed,
                       xor_expect_inv<W>(), d_want, pow_table<W>());
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : hip_fail(e, W::kKernel, "_xor_expect_kernel launch");
}

// ------------------------------------- running CRCs of an object's parts
// The tile of the scan calls in entries: a power of two, 0 = the default
// (photon_crc_set_scan_tile).
std::atomic<uint32_t> g_scan_tile{0};
// 1,024: verify's
constexpr uint32_t kScanTileDefault = 1024;

uint32_t scan_tile_now() {
    const uint32_t t = g_scan_tile.load(std::memory_order_relaxed);
    return t ? t : kScanTileDefault;
}

// photon_crc32c_scan_parts_n / photon_crc64ecma_scan_parts_n: reduce, carry
// and apply on `stream`; apply alone when everything is one tile.
template <typename W>
int scan_parts_n(const typename W::T* d_crc, const uint64_t* d_len, const uint64_t* d_obj_start, uint64_t nobj,
                 uint64_t nparts, typename W::T seed0, const typename W::T* d_seeds, typename W::T* d_run,
                 uint64_t* d_end, void* d_work, uint64_t work_bytes, void* stream) {
    typedef typename W::T T;
    typedef typename W::Pow P;
    if (!nobj || !nparts) return 0;
    if (!d_crc || !d_len || !d_run || !d_work) return fail(-EINVAL, "null part CRCs, lengths, running CRCs or workspace");
    if (!d_obj_start && nobj != 1) return fail(-EINVAL, "a null d_obj_start means one object: nobj must be 1");
    const uint32_t tile = scan_tile_now();
    const uint64_t words = scan_work_words(nparts, tile);
    if (words == kScanNone)
        return fail(-EINVAL, "too many parts: " + std::to_string(nparts) + " are more than " +
                                 std::to_string(kScanMaxParts));
    if (work_bytes < words * 8)
        return fail(-EINVAL, "workspace too small: work_bytes " + std::to_string(work_bytes) + ", needed " +
                                 std::to_string(words * 8));
    if ((uintptr_t)d_work & 7u) return fail(-EINVAL, "the workspace is not 8-byte aligned");
    int cus = 0;
    const int dev = current_device(&cus);
    if (dev < 0) return dev;
    hipStream_t st = static_cast<hipStream_t>(stream);
    uint64_t* work = static_cast<uint64_t*>(d_work);
    const ScanIn<T> in = {d_crc, d_len, d_obj_start, nobj, nparts, seed0, d_seeds};
    const uint64_t tiles = scan_tiles(nparts, tile);
    const dim3 grid(tiles < kScanMaxGrid ? (uint32_t)tiles : kScanMaxGrid), block(scan_block(tile));
    hipError_t e;
    if (tiles > 1) {
        hipLaunchKernelGGL((scan_reduce_kernel<W, P>), grid, block, 0, st, in, tile, work, pow_table<W>());
        if ((e = hipGetLastError()) != hipSuccess) return hip_fail(e, W::kKernel, " scan_reduce_kernel launch");
        hipLaunchKernelGGL(scan_carry_kernel<W>, dim3(1), dim3(kScanChunk), 0, st, work, tiles);
        if ((e = hipGetLastError()) != hipSuccess) return hip_fail(e, W::kKernel, " scan_carry_kernel launch");
    }
    hipLaunchKernelGGL((scan_apply_kernel<W, P>), grid, block, 0, st, in, tile, static_cast<const uint64_t*>(work),
                       d_run, d_end, pow_table<W>());
    e = hipGetLastError();
    return e == hipSuccess ? 0 : hip_fail(e, W::kKernel, " scan_apply_kernel launch");
}

// ------------------------------------- stored CRCs checked on the device
// The tile of the verify calls in entries: a power of two, 0 = the default
// (photon_crc_set_verify_tile).
std::atomic<uint32_t> g_verify_tile{0};
// 1,024: measured against 256, 4,096, 16,384 and 65,536 (profiles/verify_ab.jsonl)
constexpr uint32_t kVerifyTileDefault = 1024;

uint32_t verify_tile_now() {
    const uint32_t t = g_verify_tile.load(std::memory_order_relaxed);
    return t ? t : kVerifyTileDefault;
}

uint32_t verify_grid(uint64_t units) { return units < kVerifyMaxGrid ? (uint32_t)units : kVerifyMaxGrid; }

// photon_crc32c_verify_n / _verify_ptr_n and the CRC-64 forms: expected words
// by stride (d_expected) or by pointer (d_expected_ptr), the other one null.
// mark, scan and, with bad_cap > 0, list, on `stream`.
template <typename W>
int verify_n(const typename W::T* d_crc, const void* d_expected, uint64_t expected_stride,
             const void* const* d_expected_ptr, bool by_ptr, uint64_t count, photon_crc_verify_report* d_report,
             uint64_t* d_bad_idx, uint64_t bad_cap, void* d_work, uint64_t work_bytes, void* stream) {
    typedef typename W::T T;
    if (!count) return 0;
    if (!d_crc || (by_ptr ? !d_expected_ptr : !d_expected) || !d_report || !d_work || (!d_bad_idx && bad_cap))
        return fail(-EINVAL, by_ptr ? "null computed CRCs, pointer array, report, workspace or index list"
                                    : "null computed CRCs, expected words, report, workspace or index list");
    if (!by_ptr && expected_stride < sizeof(T) && count > 1)
        return fail(-EINVAL, "expected_stride " + std::to_string(expected_stride) + " is below the word width " +
                                 std::to_string(sizeof(T)));
    const uint32_t tile = verify_tile_now();
    const uint64_t words = verify_work_words(count, tile);
    if (words == kVerifyNone)
        return fail(-EINVAL, "too many entries: " + std::to_string(count) + " are more than " +
                                 std::to_string(kVerifyMaxCount));
    if (work_bytes < words * 8)
        return fail(-EINVAL, "workspace too small: work_bytes " + std::to_string(work_bytes) + ", needed " +
                                 std::to_string(words * 8));
    if ((uintptr_t)d_work & 7u) return fail(-EINVAL, "the workspace is not 8-byte aligned");
    int cus = 0;
    const int dev = current_device(&cus);
    if (dev < 0) return dev;
    hipStream_t st = static_cast<hipStream_t>(stream);
    uint64_t* work = static_cast<uint64_t*>(d_work);
    const uint64_t tiles = verify_tiles(count, tile);
    const dim3 grid(verify_grid(tiles)), block(tile < kVerifyBlock ? tile : kVerifyBlock);
    hipLaunchKernelGGL(verify_mark_kernel<T>, grid, block, 0, st, d_crc, d_expected, expected_stride, d_expected_ptr,
                       count, tile, work);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return hip_fail(e, W::kKernel, " verify_mark_kernel launch");
    hipLaunchKernelGGL(verify_scan_kernel, dim3(1), dim3(kVerifyScanBlock), 0, st, work, tiles, bad_cap,
                       reinterpret_cast<uint64_t*>(d_report));
    if ((e = hipGetLastError()) != hipSuccess) return hip_fail(e, W::kKernel, " verify_scan_kernel launch");
    if (!bad_cap) return 0;
    hipLaunchKernelGGL(verify_list_kernel<T>, grid, block, 0, st, d_crc, d_expected, expected_stride, d_expected_ptr,
                       count, tile, static_cast<const uint64_t*>(work), bad_cap, d_bad_idx);
    e = hipGetLastError();
    return e == hipSuccess ? 0 : hip_fail(e, W::kKernel, " verify_list_kernel launch");
}

// photon_crc32c_stamp_n / _stamp_ptr_n and the CRC-64 forms.
template <typename W>
int stamp_n(const typename W::T* d_crc, uint64_t count, void* d_dst, uint64_t dst_stride, void* const* d_dst_ptr,
            bool by_ptr, void* stream) {
    typedef typename W::T T;
    if (!count) return 0;
    if (!d_crc || (by_ptr ? !d_dst_ptr : !d_dst))
        return fail(-EINVAL, by_ptr ? "null CRCs or pointer array" : "null CRCs or destination");
    if (!by_ptr && dst_stride < sizeof(T) && count > 1)
        return fail(-EINVAL, "dst_stride " + std::to_string(dst_stride) + " is below the word width " +
                                 std::to_string(sizeof(T)));
    if (count > kVerifyMaxCount)
        return fail(-EINVAL, "too many entries: " + std::to_string(count) + " are more than " +
                                 std::to_string(kVerifyMaxCount));
    int cus = 0;
    const int dev = current_device(&cus);
    if (dev < 0) return dev;
    hipLaunchKernelGGL(verify_stamp_kernel<T>, dim3(verify_grid((count + kVerifyBlock - 1) / kVerifyBlock)),
                       dim3(kVerifyBlock), 0, static_cast<hipStream_t>(stream), d_crc, count, d_dst, dst_stride,
                       d_dst_ptr);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : hip_fail(e, W::kKernel, " verify_stamp_kernel launch");
}

// ------------------------------------------- many large parts
// The piece of photon_crc{32c,64ecma}_{copy,batch}_parts_n: a multiple of 4
// KiB, 0 = automatic (photon_crc_set_parts_piece).
std::atomic<uint64_t> g_parts_piece{0};
// 32 KiB: measured against 64 and 128 KiB (profiles/copy_parts_ab.jsonl)
constexpr uint64_t kPartsPieceDefault = 32u << 10;

uint64_t parts_piece_now() {
    const uint64_t p = g_parts_piece.load(std::memory_order_relaxed);
    return p ? p : kPartsPieceDefault;
}

// The plan of a call: the piece, the slots per part P and the task count;
// false when nparts * P is beyond what the kernels index.
struct PartsPlan {
    uint64_t max_bytes, piece, per_part, ntasks;
};
bool parts_plan(uint64_t nparts, uint64_t max_part_bytes, uint64_t piece, PartsPlan* pl) {
    pl->max_bytes = max_part_bytes < kPartsMaxBytes ? max_part_bytes : kPartsMaxBytes;
    pl->piece = piece;
    pl->per_part = parts_bound(pl->max_bytes, piece);
    if (nparts > kPartsMaxTasks || pl->per_part > kPartsMaxTasks / (nparts ? nparts : 1)) return false;
    pl->ntasks = nparts * pl->per_part;
    return true;
}

// K^(2^i), K = x^(8 piece), for the part fold kernel: kept per thread while
// the piece stays the same (it is a setting: every call of a process has it).
template <typename W>
const typename W::Pow& parts_pow_table(uint64_t piece) {
    thread_local uint64_t made = 0;
    thread_local typename W::Pow t;
    if (made != piece) {
        t = part_pow_table<W>(piece);
        made = piece;
    }
    return t;
}

// The second launch of a parts call: a wavefront per part folds work[] into d_out.
template <typename W>
void launch_parts_fold(const photon_crc_iovec* d_src, uint64_t nparts, const PartsPlan& pl, const typename W::T* work,
                       typename W::T seed0, const typename W::T* d_seeds, typename W::T* d_out, hipStream_t st) {
    const uint64_t wpb = kPartsFoldBlock / 64, blocks = (nparts + wpb - 1) / wpb;
    hipLaunchKernelGGL(W::kPartsFoldKernel, dim3(blocks < kPartsFoldMaxGrid ? blocks : kPartsFoldMaxGrid),
                       dim3(kPartsFoldBlock), 0, st, d_src, nparts, pl.max_bytes, pl.piece, pl.per_part, work, seed0,
                       d_seeds, d_out, parts_pow_table<W>(pl.piece), pow_table<W>());
}

// photon_crc32c_copy_parts_n / photon_crc32c_batch_parts_n and the CRC-64
// forms: the piece kernel over nparts x P tasks on the batch kernels' grid
// (lane groups by the piece size, W::copy_lanes; photon_crc_set_lanes_per_buffer
// and photon_crc_set_batch_grid apply), then the part fold kernel, both on
// `stream` inside one heavy-launch mark.
template <typename W, bool COPY>
int parts_n(const photon_crc_iovec* d_src, void* const* d_dst, uint64_t nparts, uint64_t max_part_bytes,
            typename W::T seed0, const typename W::T* d_seeds, typename W::T* d_out, void* d_work,
            uint64_t work_bytes, void* stream) {
    typedef typename W::T T;
    if (!nparts) return 0;
    if (!d_src || !d_out || !d_work || (COPY && !d_dst))
        return fail(-EINVAL, COPY ? "null descriptor array, destination array, output or workspace"
                                  : "null descriptor array, output or workspace");
    PartsPlan pl;
    if (!parts_plan(nparts, max_part_bytes, parts_piece_now(), &pl))
        return fail(-EINVAL, "too many tasks: " + std::to_string(nparts) + " parts of up to " +
                                 std::to_string(max_part_bytes) + " bytes in pieces of " +
                                 std::to_string(pl.piece) + " are more than " + std::to_string(kPartsMaxTasks));
    const uint64_t need = pl.ntasks * sizeof(T);
    if (work_bytes < need)
        return fail(-EINVAL, "workspace too small: work_bytes " + std::to_string(work_bytes) + ", needed " +
                                 std::to_string(need));
    hipStream_t st = static_cast<hipStream_t>(stream);
    typename W::Parts a{};
    a.src = d_src;
    a.dst = d_dst;
    a.nparts = nparts;
    a.max_bytes = pl.max_bytes;
    a.piece = pl.piece;
    a.per_part = pl.per_part;
    a.ntasks = pl.ntasks;
    a.work = static_cast<T*>(d_work);
    int piece_rc = 0;
    const int rc = launch_lanes<W>(pl.ntasks, W::copy_lanes(pl.piece), true, st, W::kPartsFoldLaunch,
                                   [&](auto G, dim3 grid, const typename W::Lanes& kc) {
        const auto kernel = W::template parts_kernel<decltype(G)::value, COPY>();
        if (!kernel) {
            piece_rc = fail(-ENOTSUP, "the copying CRC-64 kernels are not part of this A/B build");
            return;
        }
        hipLaunchKernelGGL(kernel, grid, dim3(kBlock), 0, st, a, kc);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) {  // no fold after a piece kernel that was not enqueued
            piece_rc = hip_fail(e, W::kKernel, "_parts_kernel launch");
            return;
        }
        launch_parts_fold<W>(d_src, nparts, pl, a.work, seed0, d_seeds, d_out, st);
    });
    return piece_rc ? piece_rc : rc;
}

// ------------------------------------------- mixed-size parts, packed tasks
// The plan of a packed call: the cap, the piece, the piece slots C and the
// workspace's layout; 0, or what is beyond the kernels' indices (1: nparts, 2: C).
struct PackedPlan {
    uint64_t max_bytes, piece, slots;
    PackedLayout at;
};
int packed_plan(uint64_t nparts, uint64_t max_part_bytes, uint64_t max_total_bytes, uint64_t piece, uint64_t word,
                PackedPlan* pl) {
    pl->max_bytes = max_part_bytes < kPartsMaxBytes ? max_part_bytes : kPartsMaxBytes;
    pl->piece = piece;
    pl->slots = packed_slots(nparts, max_total_bytes, piece);
    if (nparts > kPackedMaxParts) return 1;
    if (pl->slots > kPackedMaxSlots) return 2;
    pl->at = packed_layout(nparts, pl->slots, word);
    return 0;
}

uint32_t packed_grid(uint64_t units) { return units < kPackedMaxGrid ? (uint32_t)(units ? units : 1) : kPackedMaxGrid; }

// The four plan launches of a packed call (count, scan, first, owner); launched(what) tells whether the
// launch before it was enqueued. false: the chain ended.
template <typename L>
bool launch_packed_plan(const photon_crc_iovec* d_src, uint64_t nparts, const PackedPlan& pl, uint64_t* tilew,
                        uint64_t* first, uint32_t* owner, uint64_t* d_report, hipStream_t st, L launched) {
    const uint64_t tiles = packed_tiles(nparts);
    const dim3 tgrid(packed_grid(tiles)), block(kPackedBlock);
    hipLaunchKernelGGL(parts_packed_count_kernel, tgrid, block, 0, st, d_src, nparts, pl.max_bytes, pl.piece, tilew);
    if (!launched(" parts_packed_count_kernel launch")) return false;
    hipLaunchKernelGGL(parts_packed_scan_kernel, dim3(1), block, 0, st, tilew, tiles, nparts, pl.slots, first,
                       d_report);
    if (!launched(" parts_packed_scan_kernel launch")) return false;
    hipLaunchKernelGGL(parts_packed_first_kernel, tgrid, block, 0, st, d_src, nparts, pl.max_bytes, pl.piece,
                       static_cast<const uint64_t*>(tilew), first);
    if (!launched(" parts_packed_first_kernel launch")) return false;
    hipLaunchKernelGGL(parts_packed_owner_kernel, dim3(packed_grid((pl.slots + kPackedBlock - 1) / kPackedBlock)),
                       block, 0, st, static_cast<const uint64_t*>(first), nparts, pl.slots, owner);
    return launched(" parts_packed_owner_kernel launch");
}

// photon_crc32c_copy_parts_packed_n / photon_crc32c_batch_parts_packed_n and
// the CRC-64 forms: the four plan kernels (count, scan, first, owner), the
// piece kernel over the packed tasks on the batch kernels' grid (sized for C
// tasks: T is on the device; lane groups by the piece size as in parts_n),
// then the part fold, all on `stream` inside one heavy-launch mark. A launch
// that fails ends the chain: the later ones are not enqueued.
template <typename W, bool COPY>
int parts_packed_n(const photon_crc_iovec* d_src, void* const* d_dst, uint64_t nparts, uint64_t max_part_bytes,
                   uint64_t max_total_bytes, typename W::T seed0, const typename W::T* d_seeds, typename W::T* d_out,
                   uint64_t* d_report, void* d_work, uint64_t work_bytes, void* stream) {
    typedef typename W::T T;
    if (!nparts) return 0;
    if (!d_src || !d_out || !d_report || !d_work || (COPY && !d_dst))
        return fail(-EINVAL, COPY ? "null descriptor array, destination array, output, report or workspace"
                                  : "null descriptor array, output, report or workspace");
    PackedPlan pl;
    const int bad = packed_plan(nparts, max_part_bytes, max_total_bytes, parts_piece_now(), sizeof(T), &pl);
    if (bad == 1)
        return fail(-EINVAL, "too many parts: " + std::to_string(nparts) + " are more than " +
                                 std::to_string(kPackedMaxParts));
    if (bad)
        return fail(-EINVAL, "too many piece slots: " + std::to_string(nparts) + " parts of " +
                                 std::to_string(max_total_bytes) + " bytes in all in pieces of " +
                                 std::to_string(pl.piece) + " need " + std::to_string(pl.slots) +
                                 ", more than " + std::to_string(kPackedMaxSlots));
    if (work_bytes < pl.at.bytes)
        return fail(-EINVAL, "workspace too small: work_bytes " + std::to_string(work_bytes) + ", needed " +
                                 std::to_string(pl.at.bytes));
    if ((uintptr_t)d_work & 7u) return fail(-EINVAL, "the workspace is not 8-byte aligned");
    hipStream_t st = static_cast<hipStream_t>(stream);
    char* work = static_cast<char*>(d_work);
    uint64_t* first = reinterpret_cast<uint64_t*>(work + pl.at.first);
    uint64_t* tilew = reinterpret_cast<uint64_t*>(work + pl.at.tiles);
    uint32_t* owner = reinterpret_cast<uint32_t*>(work + pl.at.owner);
    typename W::PartsPacked a{};
    a.src = d_src;
    a.dst = d_dst;
    a.nparts = nparts;
    a.max_bytes = pl.max_bytes;
    a.piece = pl.piece;
    a.slots = pl.slots;
    a.first = first;
    a.owner = owner;
    a.work = reinterpret_cast<T*>(work + pl.at.crc);
    int chain_rc = 0;
    auto launched = [&](const char* what) {  // false: the launch before was not enqueued
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) chain_rc = hip_fail(e, W::kKernel, what);
        return e == hipSuccess;
    };
    const int rc = launch_lanes<W>(pl.slots, W::copy_lanes(pl.piece), true, st, W::kPartsPackedFoldLaunch,
                                   [&](auto G, dim3 grid, const typename W::Lanes& kc) {
        const auto kernel = W::template parts_packed_kernel<decltype(G)::value, COPY>();
        if (!kernel) {
            chain_rc = fail(-ENOTSUP, "the copying CRC-64 kernels are not part of this A/B build");
            return;
        }
        if (!launch_packed_plan(d_src, nparts, pl, tilew, first, owner, d_report, st, launched)) return;
        hipLaunchKernelGGL(kernel, grid, dim3(kBlock), 0, st, a, kc);
        if (!launched("_parts_packed_kernel launch")) return;
        const uint64_t wpb = kPartsFoldBlock / 64, blocks = (nparts + wpb - 1) / wpb;
        hipLaunchKernelGGL(W::kPartsPackedFoldKernel, dim3(blocks < kPartsFoldMaxGrid ? blocks : kPartsFoldMaxGrid),
                           dim3(kPartsFoldBlock), 0, st, d_src, nparts, pl.max_bytes, pl.piece, pl.slots,
                           static_cast<const uint64_t*>(first), static_cast<const T*>(a.work), seed0, d_seeds, d_out,
                           parts_pow_table<W>(pl.piece), pow_table<W>());
    });
    return chain_rc ? chain_rc : rc;
}

}  // namespace

// For the other translation units of the library (internal.h).
int report_error(int code, const char* what) { return fail(code, what); }
int report_hip_error(hipError_t e, const char* what) { return hip_fail(e, what); }
}  // namespace pcrc

using namespace pcrc;

extern "C" {

int photon_crc_device_count(void) {
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) return hip_fail(e, "hipGetDeviceCount");
    int ok = 0;
    for (int d = 0; d < n; ++d) {
        hipDeviceProp_t prop;
        if (hipGetDeviceProperties(&prop, d) == hipSuccess && strncmp(prop.gcnArchName, "gfx950", 6) == 0) ++ok;
    }
    if (!ok) return fail(-ENODEV, "photon_crc: no gfx950 device");
    return ok;
}

const char* photon_crc_last_error(void) { return g_err.c_str(); }

int photon_crc_set_lanes_per_buffer(int g) {
    if (g != 0 && g != 4 && g != 8 && g != 16 && g != 32 && g != 64)
        return fail(-EINVAL, "lanes per buffer must be 0, 4, 8, 16, 32 or 64");
    g_lanes_override.store(g, std::memory_order_relaxed);
    return 0;
}

int photon_crc_lanes_for(uint64_t nbytes) { return batch_lanes(nbytes); }

int photon_crc_set_batch_grid(int workgroups) {
    if (workgroups < 0) return fail(-EINVAL, "workgroups must be >= 0 (0 = one per CU)");
    g_grid_cap.store(workgroups, std::memory_order_relaxed);
    return 0;
}

void photon_crc_test_fail_next(int n) { g_fail_next = n > 0 ? n : 0; }

int photon_crc_set_mid_kernel(int on) {
    if (on != 0 && on != 1) return fail(-EINVAL, "mid kernel: 0 or 1");
    g_mid_kernel.store(on, std::memory_order_relaxed);
    return 0;
}

int photon_crc_test_tables(int which, uint32_t* out, int n) {
    if (!out) return fail(-EINVAL, "null output");
    if (which <= 3 || which == 8) {
        const int rc = host_engine_table(which, out, n);
        return rc < 0 ? fail(-EINVAL, "bad table id or short output") : rc;
    }
    if (n < 32) return fail(-EINVAL, "short output");
    if (which == 4 || which == 5) {  // device combine / trim powers x^(+-8*2^i)
        const PowTable& t = which == 4 ? pow_table<Crc32c>() : rshift_table<Crc32c>();
        for (int i = 0; i < 32; ++i) out[i] = t.x8pow2[i];
        return 32;
    }
    if (which == 6) {  // batch kernels' row shifts x^(8*16*G), G = 4, 8, 16, 32, 64
        for (int k = 0; k < 5; ++k) out[k] = lane_consts(4 << k).kshift;
        return 5;
    }
    if (which == 7) {  // lane-combine bases: image of x^0 under x^(128*2^k), k < 6
        const LaneConsts& c = lane_consts(64);
        for (int k = 0; k < 6; ++k) out[k] = c.basis[k][31];
        return 6;
    }
    if (which == 9) {  // finish tables F_d (G <= 8): image of x^0 under x^(32+128d), d < 8
        const LaneConsts& c = lane_consts(8);
        for (int d = 0; d < 8; ++d) out[d] = c.fbasis[d][31];
        return 8;
    }
    return fail(-EINVAL, "bad table id");
}

int photon_crc_test_long_plan(uint64_t addr, uint64_t n, int cus, int lanes, int rounds, int crc64, uint64_t* out,
                              int nout) {
    if (!out || cus < 1 || (lanes != 0 && lanes != 32 && lanes != 64) || rounds < 0 || rounds > 64)
        return fail(-EINVAL, "bad plan arguments");
    const LongPlan lp = long_plan_for(reinterpret_cast<const void*>(addr), n, cus,
                                      (uint32_t)lanes | (uint32_t)rounds << 8, 0, crc64 != 0);
    const LongPowers& pw = long_powers(lp, crc64 != 0);
    std::vector<uint64_t> w = {lp.head, lp.chunk, lp.nchunks, lp.last, lp.rounds, lp.grid, lp.stride, lp.lead,
                               (uint64_t)lp.lanes};
    if (crc64) {
        w.insert(w.end(), pw.xsb64, pw.xsb64 + 64);
        w.push_back(pw.x64);
        w.insert(w.end(), pw.zt64, pw.zt64 + 16);
        w.insert(w.end(), pw.ft64, pw.ft64 + lp.grid);
    } else {
        w.insert(w.end(), pw.xsb32, pw.xsb32 + 32);
        w.insert(w.end(), pw.xb32, pw.xb32 + 32);
        w.insert(w.end(), pw.zt32, pw.zt32 + 16);
        w.insert(w.end(), pw.ft32, pw.ft32 + lp.grid);
    }
    if ((int)w.size() > nout) return fail(-EINVAL, "short output");
    memcpy(out, w.data(), w.size() * 8);
    return (int)w.size();
}

int photon_crc_test_small_plan(uint64_t addr, uint64_t n, int crc64, uint64_t* out, int nout) {
    if (!out) return fail(-EINVAL, "null output");
    const void* p = reinterpret_cast<const void*>(addr);
    return crc64 ? test_small_plan<Crc64>(p, n, out, nout) : test_small_plan<Crc32c>(p, n, out, nout);
}

int photon_crc_set_generic_rows(int rows_per_step) {
    if (rows_per_step != -1 && rows_per_step != 2 && rows_per_step != 4 && rows_per_step != 8)
        return fail(-EINVAL, "rows per step must be -1 (auto), 2, 4 or 8");
    g_generic_u.store(rows_per_step, std::memory_order_relaxed);
    return 0;
}

int photon_crc_set_msg_mode(int mode) {
    if (mode < 0 || mode > 2) return fail(-EINVAL, "message mode must be 0 (auto), 1 (fused) or 2 (two kernels)");
    g_msg_mode.store(mode, std::memory_order_relaxed);
    return 0;
}

int photon_crc_set_long_shape(int lanes, int rounds) {
    if ((lanes != 0 && lanes != 32 && lanes != 64) || rounds < 0 || rounds > 64)
        return fail(-EINVAL, "long-buffer lanes must be 0, 32 or 64 and rounds 0..64");
    g_long_shape.store((uint32_t)lanes | (uint32_t)rounds << 8, std::memory_order_relaxed);
    return 0;
}

int photon_crc64_set_full_rows(int mode, int rows_per_step) {
    if (mode < 0 || mode > 3 || (rows_per_step != 2 && rows_per_step != 4))
        return fail(-EINVAL, "full-row mode must be 0..3 and rows per step 2 or 4");
    g_full64.store((uint32_t)rows_per_step << 4 | (uint32_t)mode, std::memory_order_relaxed);
    return 0;
}

int photon_crc_set_routed_wait(int spin_us, int sleep_ahead) {
    if (spin_us < 0 || spin_us > 65535) return fail(-EINVAL, "spin window must be 0..65535 us");
    g_routed_wait.store((uint32_t)spin_us | (sleep_ahead ? 1u << 16 : 0u), std::memory_order_relaxed);
    return 0;
}

int photon_crc_set_small_service(int idle_us) {
    if (idle_us < 0 || idle_us > 1000000) return fail(-EINVAL, "service idle time must be 0..1000000 us");
    g_svc_idle_us.store(idle_us, std::memory_order_relaxed);
    if (idle_us == 0) service_end_all();  // idle times of running launches stay as they were started
    return 0;
}

int photon_crc_set_small_service_life(int life_us) {
    if (life_us < 100 || life_us > 1000000) return fail(-EINVAL, "service life must be 100..1000000 us");
    g_svc_life_us.store(life_us, std::memory_order_relaxed);
    return 0;
}

int photon_crc_set_service_doorbell(int bar) {
    if (bar != 0 && bar != 1) return fail(-EINVAL, "doorbell must be 0 (pinned host) or 1 (device BAR)");
    service_end_all();  // launches from now on pick the doorbell
    g_svc_bell.store(bar, std::memory_order_relaxed);
    return 0;
}

int photon_crc_small_service_doorbell(int kind) {
    if (kind != 0 && kind != 1) return fail(-EINVAL, "kind must be 0 (CRC-32C) or 1 (CRC-64)");
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return fail(-ENODEV, "no device");
    return service_doorbell_of(dev, kind);
}

uint64_t photon_crc_small_service_deferred(void) { return g_svc_deferred.load(std::memory_order_relaxed); }

int photon_crc_small_service_stats(uint64_t* served, uint64_t* starts, uint64_t* missed) {
    if (served) *served = g_svc_served.load(std::memory_order_relaxed);
    if (starts) *starts = g_svc_starts.load(std::memory_order_relaxed);
    if (missed) *missed = g_svc_missed.load(std::memory_order_relaxed);
    return 0;
}

int photon_crc_set_msg_rows(int rows_per_step) {
    if (rows_per_step != 2 && rows_per_step != 4) return fail(-EINVAL, "message rows per step must be 2 or 4");
    g_msg_u.store(rows_per_step, std::memory_order_relaxed);
    return 0;
}

int photon_crc32c_batch_strided(const void* d_base, uint64_t stride, uint64_t nbytes, uint64_t count,
                                uint32_t seed0, const uint32_t* d_seeds, uint32_t* d_out, void* stream) {
    return batch_strided<Crc32c>(d_base, stride, nbytes, count, seed0, d_seeds, d_out, stream);
}

int photon_crc32c_batch_strided_sync(const void* d_base, uint64_t stride, uint64_t nbytes, uint64_t count,
                                     uint32_t seed0, const uint32_t* d_seeds, uint32_t* d_out, void* stream) {
    int rc = photon_crc32c_batch_strided(d_base, stride, nbytes, count, seed0, d_seeds, d_out, stream);
    if (rc) return rc;
    hipError_t e = hipStreamSynchronize(static_cast<hipStream_t>(stream));
    if (e != hipSuccess) return hip_fail(e, "hipStreamSynchronize");
    return 0;
}

}  // extern "C"

namespace pcrc {
namespace {

// The host-memory pipeline for CRC word type T (uint32_t CRC-32C, uint64_t
// CRC-64/ECMA); `device_batch` is the matching strided device batch.
template <typename T>
int host_batch_impl(const void* h_base, uint64_t stride, uint64_t nbytes, uint64_t count, T seed0, const T* h_seeds,
                    T* h_out,
                    int (*device_batch)(const void*, uint64_t, uint64_t, uint64_t, T, const T*, T*, void*)) {
    if (!count) return 0;
    if (!h_out || (!h_base && nbytes) || stride < nbytes) return fail(-EINVAL, "bad arguments");
    if (!nbytes) {  // crc32c_extend / crc64ecma_extend over 0 bytes return the seed (crc.cpp:340)
        for (uint64_t i = 0; i < count; ++i) h_out[i] = h_seeds ? h_seeds[i] : seed0;
        return 0;
    }
    // pitch > kStageBytes, asked of nbytes (kStageBytes is a multiple of 256) so that no size wraps the pitch
    if (nbytes > kStageBytes) return fail(-EINVAL, "buffer larger than a staging chunk (256 MiB)");
    const uint64_t span = g_host_stage.load(std::memory_order_relaxed);
    const StagePlan pl = stage_plan(nbytes, count, span ? span : kStageBytes);
    const uint64_t pitch = pl.pitch;
    int cus = 0;
    int dev = current_device(&cus);
    if (dev < 0) return dev;
    if (dev >= kMaxDevices) return fail(-ENODEV, "device index beyond the pipeline table");
    HostPipe* p = &g_pipes[dev];
    std::lock_guard<std::mutex> lk(p->mu);
    int rc = pipe_init(*p);
    if (rc) return rc;
    // Any return after the first enqueue drains both streams first: copies
    // from the caller's h_base and kernels writing p->d_out must not outlive
    // the call (the caller may free h_base; the next call reuses the slots).
    struct Drain {
        HostPipe* p;
        ~Drain() {
            (void)hipStreamSynchronize(p->copy);
            (void)hipStreamSynchronize(p->comp);
        }
    } drain{p};
    hipError_t e;
    const uint64_t bytes = count * sizeof(T);
    if (p->out_cap < bytes) {
        services_end_before_free();
        if (p->d_out) (void)hipFree(p->d_out);
        if (p->d_seeds) (void)hipFree(p->d_seeds);
        p->d_out = p->d_seeds = nullptr;
        p->out_cap = 0;
        if ((e = hipMalloc(&p->d_out, bytes)) != hipSuccess) return hip_fail(e, "hipMalloc(out)");
        if ((e = hipMalloc(&p->d_seeds, bytes)) != hipSuccess) return hip_fail(e, "hipMalloc(seeds)");
        p->out_cap = bytes;
    }
    T* d_out = static_cast<T*>(p->d_out);
    T* d_seeds = static_cast<T*>(p->d_seeds);
    if (h_seeds) {
        e = hipMemcpyAsync(d_seeds, h_seeds, bytes, hipMemcpyHostToDevice, p->comp);
        if (e != hipSuccess) return hip_fail(e, "seeds H2D");
    }
    const uint8_t* src = static_cast<const uint8_t*>(h_base);
    for (uint64_t i = 0; i < pl.nchunks; ++i) {
        const StageChunk ch = stage_chunk(pl, i);
        const int slot = ch.slot;
        const uint64_t first = ch.first, k = ch.k;
        if ((e = hipStreamWaitEvent(p->copy, p->consumed[slot], 0)) != hipSuccess) return hip_fail(e, "wait");
        e = hipMemcpy2DAsync(p->stage[slot], pitch, src + first * stride, stride, nbytes, k, hipMemcpyHostToDevice,
                             p->copy);
        if (e != hipSuccess) return hip_fail(e, "hipMemcpy2DAsync H2D");
        if ((e = hipEventRecord(p->copied[slot], p->copy)) != hipSuccess) return hip_fail(e, "record");
        if ((e = hipStreamWaitEvent(p->comp, p->copied[slot], 0)) != hipSuccess) return hip_fail(e, "wait");
        rc = device_batch(p->stage[slot], pitch, nbytes, k, seed0, h_seeds ? d_seeds + first : nullptr, d_out + first,
                          p->comp);
        if (rc) return rc;
        if ((e = hipEventRecord(p->consumed[slot], p->comp)) != hipSuccess) return hip_fail(e, "record");
    }
    e = hipMemcpyAsync(h_out, d_out, bytes, hipMemcpyDeviceToHost, p->comp);
    if (e != hipSuccess) return hip_fail(e, "out D2H");
    e = hipStreamSynchronize(p->comp);
    if (e != hipSuccess) return hip_fail(e, "hipStreamSynchronize");
    return 0;
}

}  // namespace
}  // namespace pcrc

extern "C" {

int photon_crc32c_host_batch_strided(const void* h_base, uint64_t stride, uint64_t nbytes, uint64_t count,
                                     uint32_t seed0, const uint32_t* h_seeds, uint32_t* h_out) {
    return host_batch_impl<uint32_t>(h_base, stride, nbytes, count, seed0, h_seeds, h_out,
                                     &photon_crc32c_batch_strided);
}

int photon_crc64ecma_host_batch_strided(const void* h_base, uint64_t stride, uint64_t nbytes, uint64_t count,
                                        uint64_t seed0, const uint64_t* h_seeds, uint64_t* h_out) {
    return host_batch_impl<uint64_t>(h_base, stride, nbytes, count, seed0, h_seeds, h_out,
                                     &photon_crc64ecma_batch_strided);
}

// The gfx950 devices of this process, in id order (at most kMaxDevices).
static int usable_devices(std::vector<int>* devs) {
    int total = 0;
    hipError_t e = hipGetDeviceCount(&total);
    if (e != hipSuccess) return hip_fail(e, "hipGetDeviceCount");
    devs->clear();
    for (int d = 0; d < total && d < kMaxDevices; ++d) {
        hipDeviceProp_t prop;
        if (hipGetDeviceProperties(&prop, d) == hipSuccess && strncmp(prop.gcnArchName, "gfx950", 6) == 0)
            devs->push_back(d);
    }
    return devs->empty() ? fail(-ENODEV, "photon_crc: no gfx950 device") : 0;
}

int photon_crc32c_host_batch_strided_multi(const void* h_base, uint64_t stride, uint64_t nbytes, uint64_t count,
                                           uint32_t seed0, const uint32_t* h_seeds, uint32_t* h_out, int ndev) {
    if (!count) return 0;
    if (!h_out || (!h_base && nbytes) || stride < nbytes) return fail(-EINVAL, "bad arguments");
    std::vector<int> usable;
    if (int rc = usable_devices(&usable)) return rc;
    // Contiguous slices of the buffer indices (multi_device.h shard_plan), one
    // host thread per device, each driving that device's pipeline over its own
    // host link.
    const std::vector<Slice> plan = shard_plan(count, first_devices(usable, ndev));
    const uint8_t* src = static_cast<const uint8_t*>(h_base);
    HipRT rt;
    std::string err;
    const int rc = run_slices_threaded(
        rt, plan,
        [&](const Slice& sl) {
            return photon_crc32c_host_batch_strided(src + sl.lo * stride, stride, nbytes, sl.hi - sl.lo, seed0,
                                                    h_seeds ? h_seeds + sl.lo : nullptr, h_out + sl.lo);
        },
        [] { return g_err; }, &err);
    return rc ? fail(rc, err) : 0;
}

int photon_crc32c_batch_strided_shards(const photon_crc_shard* shards, int nshards) {
    if (nshards < 0 || (nshards && !shards)) return fail(-EINVAL, "bad shard list");
    HipRT rt;
    return run_on_devices(
        rt, nshards, [&](int i) { return shards[i].device; },
        [&](int i) {
            const photon_crc_shard& s = shards[i];
            return photon_crc32c_batch_strided(s.d_base, s.stride, s.nbytes, s.count, s.seed0, s.d_seeds, s.d_out,
                                               s.stream);
        },
        nullptr);
}

int photon_crc32c_batch_iov(const photon_crc_iovec* d_iov, uint64_t count, uint32_t seed0,
                            const uint32_t* d_seeds, uint32_t* d_out, void* stream) {
    return batch_iov<Crc32c>(d_iov, count, seed0, d_seeds, d_out, stream);
}

int photon_crc32c_batch_msg(const photon_crc_iovec* d_iov, const uint64_t* d_msg_start, uint64_t nmsg,
                            uint32_t seed0, const uint32_t* d_seeds, uint32_t* d_seg_out, uint32_t* d_out,
                            void* stream) {
    if (!nmsg) return 0;
    if (!d_iov || !d_msg_start || !d_out) return fail(-EINVAL, "null argument");
    hipStream_t st = static_cast<hipStream_t>(stream);
    uint64_t nseg = 0;
    hipError_t e = hipMemcpyAsync(&nseg, d_msg_start + nmsg, sizeof(nseg), hipMemcpyDeviceToHost, st);
    if (e != hipSuccess) return hip_fail(e, "hipMemcpyAsync(msg_start)");
    e = hipStreamSynchronize(st);
    if (e != hipSuccess) return hip_fail(e, "hipStreamSynchronize");
    return photon_crc32c_batch_msg_n(d_iov, d_msg_start, nmsg, nseg, seed0, d_seeds, d_seg_out, d_out, stream);
}

}  // extern "C"

// Messages with an explicit lane-group size (0 = automatic): segments in host
// memory read by the kernels over the host link go faster with wide groups
// (longer contiguous requests), see checked_batch.cpp.
int pcrc::batch_msg_lanes(const photon_crc_iovec* d_iov, const uint64_t* d_msg_start, uint64_t nmsg, uint64_t nseg,
                          uint32_t seed0, const uint32_t* d_seeds, uint32_t* d_seg_out, uint32_t* d_out,
                          void* stream, int lanes, uint32_t* seg_scratch) {
    if (!nmsg) return 0;
    if (!d_iov || !d_msg_start || !d_out) return fail(-EINVAL, "null argument");
    hipStream_t st = static_cast<hipStream_t>(stream);
    hipError_t e;
    BatchArgs a{};
    a.iov = d_iov;
    a.count = nseg;
    a.out = d_seg_out;
    a.seed0 = 0;
    // One kernel (a group per message) when there are enough messages to fill
    // the chip and messages are short; else segment CRCs in parallel + a fold
    // kernel (few, long messages).
    const int g = lanes ? lanes : choose_lanes(8192);
    const uint64_t gpw = 64 / (uint64_t)g;
    // (With per-segment CRCs requested the fused form folds with the group-
    // spread multiply of crc32c_batch_kernel<G, U, 2>.)
    const int mode = g_msg_mode.load(std::memory_order_relaxed);
    const bool fused = mode == 1 || (mode == 0 && nmsg >= 4096 * gpw && nseg <= 64 * nmsg);
    if (fused) {
        a.msg_start = d_msg_start;
        a.nmsg = nmsg;
        a.msg_out = d_out;
        a.seeds = d_seeds;
        a.seed0 = seed0;
        const int rows_per_step = g_msg_u.load(std::memory_order_relaxed);
        // capped = false: photon_crc_set_batch_grid does not apply to the fused message form
        return launch_lanes<Crc32c>(nmsg, g, false, st, "crc32c_batch_kernel<msg> launch",
                                    [&](auto G, dim3 grid, const LaneConsts& kc) {
            auto rows = [&](auto U) {
                constexpr int GG = decltype(G)::value, UU = decltype(U)::value;
                if (a.out)
                    hipLaunchKernelGGL((crc32c_batch_kernel<GG, UU, 2>), grid, dim3(kBlock), 0, st, a, kc,
                                       pow_table<Crc32c>());
                else
                    hipLaunchKernelGGL((crc32c_batch_kernel<GG, UU, 1>), grid, dim3(kBlock), 0, st, a, kc,
                                       pow_table<Crc32c>());
            };
            if (rows_per_step == 2)
                rows(Int<2>{});
            else
                rows(Int<4>{});
        });
    }
    void* scratch = nullptr;  // segment CRCs the caller did not ask for
    if (!d_seg_out && nseg && seg_scratch) {
        a.out = seg_scratch;
    } else if (!d_seg_out && nseg) {
        if (int rc = scratch_alloc(&scratch, nseg * 4, st)) return rc;
        a.out = static_cast<uint32_t*>(scratch);
    }
    int rc = launch_batch(a, 8192, st, lanes);
    if (!rc) {
        const int bs = 256;
        hipLaunchKernelGGL(crc32c_msg_fold_kernel, dim3((nmsg + bs - 1) / bs), dim3(bs), 0, st, d_iov, d_msg_start,
                           nmsg, a.out, seed0, d_seeds, d_out, pow_table<Crc32c>());
        e = hipGetLastError();
        if (e != hipSuccess) rc = hip_fail(e, "crc32c_msg_fold_kernel launch");
    }
    if (scratch) {
        const int frc = scratch_free(scratch, st);
        if (!rc) rc = frc;
    }
    return rc;
}

extern "C" {

int photon_crc32c_batch_msg_n(const photon_crc_iovec* d_iov, const uint64_t* d_msg_start, uint64_t nmsg,
                              uint64_t nseg, uint32_t seed0, const uint32_t* d_seeds, uint32_t* d_seg_out,
                              uint32_t* d_out, void* stream) {
    return pcrc::batch_msg_lanes(d_iov, d_msg_start, nmsg, nseg, seed0, d_seeds, d_seg_out, d_out, stream, 0);
}

// Copy + CRC-32C in one pass (crc32c_gpu.h; DESIGN.md "Copy + CRC").
int photon_crc32c_copy_batch_strided(const void* src_base, uint64_t src_stride, void* d_dst_base,
                                     uint64_t dst_stride, uint64_t nbytes, uint64_t count, uint32_t seed0,
                                     const uint32_t* d_seeds, uint32_t* d_out, void* stream) {
    return copy_batch_strided<Crc32c>(src_base, src_stride, d_dst_base, dst_stride, nbytes, count, seed0, d_seeds,
                                      d_out, stream);
}

int photon_crc32c_copy_batch_iov(const photon_crc_iovec* d_src, void* const* d_dst, uint64_t count, uint32_t seed0,
                                 const uint32_t* d_seeds, uint32_t* d_out, void* stream) {
    return copy_batch_iov<Crc32c>(d_src, d_dst, count, seed0, d_seeds, d_out, stream);
}

int photon_crc32c_gather_msg_n(const photon_crc_iovec* d_iov, const uint64_t* d_msg_start, uint64_t nmsg,
                               uint64_t nseg, void* const* d_dst, uint32_t seed0, const uint32_t* d_seeds,
                               uint32_t* d_seg_out, uint32_t* d_out, void* stream) {
    if (!nmsg) return 0;
    if (!d_msg_start || !d_dst || !d_out || (!d_iov && nseg)) return fail(-EINVAL, "null argument");
    // Always the one-kernel form (a lane group walks its message's segments
    // and keeps the running destination); lane groups as batch_msg_n takes.
    CopyBatchArgs a{};
    a.iov = d_iov;
    a.count = nseg;
    a.out = d_seg_out;
    a.msg_start = d_msg_start;
    a.nmsg = nmsg;
    a.msg_out = d_out;
    a.seeds = d_seeds;
    a.seed0 = seed0;
    a.dst = d_dst;
    return launch_copy(a, nmsg, choose_lanes(8192), static_cast<hipStream_t>(stream), d_seg_out ? 2 : 1);
}

int photon_crc32c_copy_msg_iov_n(const photon_crc_iovec* d_src, const uint64_t* d_src_start, uint64_t nsrc,
                                 const photon_crc_iovec* d_dst, const uint64_t* d_dst_start, uint64_t ndst,
                                 uint64_t nmsg, const uint64_t* d_size, uint32_t seed0, const uint32_t* d_seeds,
                                 uint32_t* d_out, uint64_t* d_copied, void* stream) {
    return copy_msg_iov_n<Crc32c>(d_src, d_src_start, nsrc, d_dst, d_dst_start, ndst, nmsg, d_size, seed0, d_seeds,
                                  d_out, d_copied, stream);
}

int photon_crc32c_copy_msg_iov_seg_n(const photon_crc_iovec* d_src, const uint64_t* d_src_start, uint64_t nsrc,
                                     const photon_crc_iovec* d_dst, const uint64_t* d_dst_start, uint64_t ndst,
                                     uint64_t nmsg, const uint64_t* d_size, uint32_t seed0, const uint32_t* d_seeds,
                                     int seg_side, uint32_t* d_seg_out, uint32_t* d_out, uint64_t* d_copied,
                                     void* stream) {
    if (!nmsg) return 0;
    if (!d_src_start || !d_dst_start || !d_out || !d_seg_out || (!d_src && nsrc) || (!d_dst && ndst))
        return fail(-EINVAL, "null argument");
    if (seg_side != PHOTON_CRC_SEG_OF_SRC && seg_side != PHOTON_CRC_SEG_OF_DST)
        return fail(-EINVAL, "seg_side is neither PHOTON_CRC_SEG_OF_SRC nor PHOTON_CRC_SEG_OF_DST");
    CopyIovSegArgs a{};
    a.src = d_src;
    a.src_start = d_src_start;
    a.dst = d_dst;
    a.dst_start = d_dst_start;
    a.nmsg = nmsg;
    a.size = d_size;
    a.seeds = d_seeds;
    a.seg_out = d_seg_out;
    a.out = d_out;
    a.copied = d_copied;
    a.seed0 = seed0;
    return launch_copy_iov_seg(a, seg_side == PHOTON_CRC_SEG_OF_DST, choose_lanes(8192),
                               static_cast<hipStream_t>(stream));
}

int photon_crc32c_copy_msg_iov_seg2_n(const photon_crc_iovec* d_src, const uint64_t* d_src_start, uint64_t nsrc,
                                      const photon_crc_iovec* d_dst, const uint64_t* d_dst_start, uint64_t ndst,
                                      uint64_t nmsg, const uint64_t* d_size, uint32_t seed0, const uint32_t* d_seeds,
                                      uint32_t* d_src_seg_out, uint32_t* d_dst_seg_out, uint32_t* d_out,
                                      uint64_t* d_copied, void* stream) {
    return copy_msg_iov_seg2_n<Crc32c>(d_src, d_src_start, nsrc, d_dst, d_dst_start, ndst, nmsg, d_size, seed0,
                                       d_seeds, d_src_seg_out, d_dst_seg_out, d_out, d_copied, stream);
}

uint64_t photon_crc_window_work_bytes(uint64_t nmsg) { return 16 * nmsg; }

int photon_crc32c_copy_msg_iov_window_n(const photon_crc_iovec* d_src, const uint64_t* d_src_start, uint64_t nsrc,
                                        const photon_crc_iovec* d_dst, const uint64_t* d_dst_start, uint64_t ndst,
                                        uint64_t nmsg, const uint64_t* d_skip, const uint64_t* d_size, uint32_t seed0,
                                        const uint32_t* d_seeds, uint32_t* d_src_seg_out, uint32_t* d_out,
                                        uint64_t* d_copied, void* d_work, void* stream) {
    return copy_msg_iov_window_n<Crc32c>(d_src, d_src_start, nsrc, d_dst, d_dst_start, ndst, nmsg, d_skip, d_size,
                                         seed0, d_seeds, d_src_seg_out, d_out, d_copied, d_work, stream);
}

int photon_crc64ecma_batch_strided(const void* d_base, uint64_t stride, uint64_t nbytes, uint64_t count,
                                   uint64_t seed0, const uint64_t* d_seeds, uint64_t* d_out, void* stream) {
    return batch_strided<Crc64>(d_base, stride, nbytes, count, seed0, d_seeds, d_out, stream);
}

int photon_crc64ecma_batch_iov(const photon_crc_iovec* d_iov, uint64_t count, uint64_t seed0,
                               const uint64_t* d_seeds, uint64_t* d_out, void* stream) {
    return batch_iov<Crc64>(d_iov, count, seed0, d_seeds, d_out, stream);
}

int photon_crc64ecma_combine_batch(const uint64_t* d_crc1, const uint64_t* d_crc2, const uint32_t* d_len2,
                                   uint64_t count, uint64_t* d_out, void* stream) {
    return combine_batch<Crc64>(d_crc1, d_crc2, d_len2, count, d_out, stream);
}

int photon_crc64ecma_trim_batch(const photon_crc64_component* d_all, const photon_crc64_component* d_prefix,
                                const photon_crc64_component* d_suffix, uint64_t count, uint64_t* d_out,
                                uint32_t* d_nerr, void* stream) {
    return trim_batch<Crc64>(d_all, d_prefix, d_suffix, count, d_out, d_nerr, stream);
}

int photon_crc64ecma_batch_msg_n(const photon_crc_iovec* d_iov, const uint64_t* d_msg_start, uint64_t nmsg,
                                 uint64_t nseg, uint64_t seed0, const uint64_t* d_seeds, uint64_t* d_seg_out,
                                 uint64_t* d_out, void* stream) {
    if (!nmsg) return 0;
    if (!d_iov || !d_msg_start || !d_out) return fail(-EINVAL, "null argument");
    hipStream_t st = static_cast<hipStream_t>(stream);
    // d_seg_out is optional: without it the segment CRCs live in stream-ordered scratch.
    void* scratch = nullptr;
    if (!d_seg_out) {
        if (int rc = scratch_alloc(&scratch, (nseg ? nseg : 1) * sizeof(uint64_t), st)) return rc;
        d_seg_out = static_cast<uint64_t*>(scratch);
    }
    Batch64Args a{};
    a.iov = d_iov;
    a.count = nseg;
    a.out = d_seg_out;
    a.seed0 = 0;
    int rc = launch_batch(a, 8192, st);
    if (!rc) {
        hipLaunchKernelGGL(crc64_msg_fold_kernel, dim3((nmsg + 255) / 256), dim3(256), 0, st, d_iov, d_msg_start,
                           nmsg, d_seg_out, seed0, d_seeds, d_out, pow_table<Crc64>());
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) rc = hip_fail(e, "crc64_msg_fold_kernel launch");
    }
    if (scratch) {
        const int frc = scratch_free(scratch, st);
        if (!rc) rc = frc;
    }
    return rc;
}

// Copy + CRC-64/ECMA in one pass (crc32c_gpu.h).
int photon_crc64ecma_copy_batch_strided(const void* src_base, uint64_t src_stride, void* d_dst_base,
                                        uint64_t dst_stride, uint64_t nbytes, uint64_t count, uint64_t seed0,
                                        const uint64_t* d_seeds, uint64_t* d_out, void* stream) {
    return copy_batch_strided<Crc64>(src_base, src_stride, d_dst_base, dst_stride, nbytes, count, seed0, d_seeds,
                                     d_out, stream);
}

int photon_crc64ecma_copy_batch_iov(const photon_crc_iovec* d_src, void* const* d_dst, uint64_t count,
                                    uint64_t seed0, const uint64_t* d_seeds, uint64_t* d_out, void* stream) {
    return copy_batch_iov<Crc64>(d_src, d_dst, count, seed0, d_seeds, d_out, stream);
}

int photon_crc64ecma_gather_msg_n(const photon_crc_iovec* d_iov, const uint64_t* d_msg_start, uint64_t nmsg,
                                  uint64_t nseg, void* const* d_dst, uint64_t seed0, const uint64_t* d_seeds,
                                  uint64_t* d_seg_out, uint64_t* d_out, void* stream) {
    if (!nmsg) return 0;
    if (!d_msg_start || !d_dst || !d_out || (!d_iov && nseg)) return fail(-EINVAL, "null argument");
    hipStream_t st = static_cast<hipStream_t>(stream);
    // One payload-reading kernel (a lane group walks its message's segments
    // and keeps the running destination). Without d_seg_out it chains the
    // register and writes d_out; with it, the segment CRCs are folded by
    // crc64_msg_fold_kernel as in photon_crc64ecma_batch_msg_n. No scratch.
    CopyBatch64Args a{};
    a.iov = d_iov;
    a.count = nseg;
    a.out = d_out;
    a.seg_out = d_seg_out;
    a.msg_start = d_msg_start;
    a.nmsg = nmsg;
    a.seeds = d_seeds;
    a.seed0 = seed0;
    a.dst = d_dst;
    int rc = launch_copy(a, nmsg, choose_lanes(8192), st, /*gather=*/true);
    if (!rc && d_seg_out) {
        hipLaunchKernelGGL(crc64_msg_fold_kernel, dim3((nmsg + 255) / 256), dim3(256), 0, st, d_iov, d_msg_start,
                           nmsg, d_seg_out, seed0, d_seeds, d_out, pow_table<Crc64>());
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) rc = hip_fail(e, "crc64_msg_fold_kernel launch");
    }
    return rc;
}

int photon_crc64ecma_copy_msg_iov_n(const photon_crc_iovec* d_src, const uint64_t* d_src_start, uint64_t nsrc,
                                    const photon_crc_iovec* d_dst, const uint64_t* d_dst_start, uint64_t ndst,
                                    uint64_t nmsg, const uint64_t* d_size, uint64_t seed0, const uint64_t* d_seeds,
                                    uint64_t* d_out, uint64_t* d_copied, void* stream) {
    return copy_msg_iov_n<Crc64>(d_src, d_src_start, nsrc, d_dst, d_dst_start, ndst, nmsg, d_size, seed0, d_seeds,
                                 d_out, d_copied, stream);
}

int photon_crc64ecma_copy_msg_iov_seg_n(const photon_crc_iovec* d_src, const uint64_t* d_src_start, uint64_t nsrc,
                                        const photon_crc_iovec* d_dst, const uint64_t* d_dst_start, uint64_t ndst,
                                        uint64_t nmsg, const uint64_t* d_size, uint64_t seed0,
                                        const uint64_t* d_seeds, int seg_side, uint64_t* d_seg_out, uint64_t* d_out,
                                        uint64_t* d_copied, void* stream) {
    if (!nmsg) return 0;
    if (!d_src_start || !d_dst_start || !d_out || !d_seg_out || (!d_src && nsrc) || (!d_dst && ndst))
        return fail(-EINVAL, "null argument");
    if (seg_side != PHOTON_CRC_SEG_OF_SRC && seg_side != PHOTON_CRC_SEG_OF_DST)
        return fail(-EINVAL, "seg_side is neither PHOTON_CRC_SEG_OF_SRC nor PHOTON_CRC_SEG_OF_DST");
    CopyIovSeg64Args a{};
    a.src = d_src;
    a.src_start = d_src_start;
    a.dst = d_dst;
    a.dst_start = d_dst_start;
    a.nmsg = nmsg;
    a.size = d_size;
    a.seg_out = d_seg_out;
    a.copied = d_copied;
    return launch_copy_iov_seg(a, seg_side == PHOTON_CRC_SEG_OF_DST, seed0, d_seeds, d_out, choose_lanes(8192),
                               static_cast<hipStream_t>(stream));
}

int photon_crc64ecma_copy_msg_iov_seg2_n(const photon_crc_iovec* d_src, const uint64_t* d_src_start, uint64_t nsrc,
                                         const photon_crc_iovec* d_dst, const uint64_t* d_dst_start, uint64_t ndst,
                                         uint64_t nmsg, const uint64_t* d_size, uint64_t seed0,
                                         const uint64_t* d_seeds, uint64_t* d_src_seg_out, uint64_t* d_dst_seg_out,
                                         uint64_t* d_out, uint64_t* d_copied, void* stream) {
    return copy_msg_iov_seg2_n<Crc64>(d_src, d_src_start, nsrc, d_dst, d_dst_start, ndst, nmsg, d_size, seed0,
                                      d_seeds, d_src_seg_out, d_dst_seg_out, d_out, d_copied, stream);
}

int photon_crc64ecma_copy_msg_iov_window_n(const photon_crc_iovec* d_src, const uint64_t* d_src_start, uint64_t nsrc,
                                           const photon_crc_iovec* d_dst, const uint64_t* d_dst_start, uint64_t ndst,
                                           uint64_t nmsg, const uint64_t* d_skip, const uint64_t* d_size,
                                           uint64_t seed0, const uint64_t* d_seeds, uint64_t* d_src_seg_out,
                                           uint64_t* d_out, uint64_t* d_copied, void* d_work, void* stream) {
    return copy_msg_iov_window_n<Crc64>(d_src, d_src_start, nsrc, d_dst, d_dst_start, ndst, nmsg, d_skip, d_size,
                                        seed0, d_seeds, d_src_seg_out, d_out, d_copied, d_work, stream);
}

int photon_crc64ecma_extend_device(const void* d_data, uint64_t nbytes, uint64_t seed, uint64_t* d_out,
                                   void* stream) {
    return extend_device<Crc64>(d_data, nbytes, seed, d_out, stream);
}

int photon_crc64ecma_copy_extend_device(const void* src, void* d_dst, uint64_t nbytes, uint64_t seed, uint64_t* d_out,
                                        void* stream) {
    return copy_extend_device<Crc64>(src, d_dst, nbytes, seed, d_out, stream);
}

int photon_crc32c_combine_batch(const uint32_t* d_crc1, const uint32_t* d_crc2, const uint32_t* d_len2,
                                uint64_t count, uint32_t* d_out, void* stream) {
    return combine_batch<Crc32c>(d_crc1, d_crc2, d_len2, count, d_out, stream);
}

int photon_crc32c_series_device(const void* d_buffer, uint32_t part_size, uint32_t n_parts, uint32_t* d_crc_parts,
                                void* stream) {
    return series_device<Crc32c>(d_buffer, part_size, n_parts, d_crc_parts, stream);
}

int photon_crc32c_combine_series_device(const uint32_t* d_crc, uint32_t part_size, uint32_t n_parts,
                                        uint32_t* d_result, void* stream) {
    return combine_series_device<Crc32c>(d_crc, part_size, n_parts, d_result, stream);
}

int photon_crc64ecma_series_device(const void* d_buffer, uint32_t part_size, uint32_t n_parts, uint64_t* d_crc_parts,
                                   void* stream) {
    return series_device<Crc64>(d_buffer, part_size, n_parts, d_crc_parts, stream);
}

int photon_crc64ecma_combine_series_device(const uint64_t* d_crc, uint32_t part_size, uint32_t n_parts,
                                           uint64_t* d_result, void* stream) {
    return combine_series_device<Crc64>(d_crc, part_size, n_parts, d_result, stream);
}

int photon_crc32c_fold_parts_n(const uint32_t* d_crc, const uint64_t* d_len, const uint64_t* d_obj_start,
                               uint64_t nobj, uint64_t nparts, uint32_t seed0, const uint32_t* d_seeds,
                               uint32_t* d_out, uint64_t* d_total, void* stream) {
    return fold_parts_n<Crc32c>(d_crc, d_len, d_obj_start, nobj, nparts, seed0, d_seeds, d_out, d_total, stream);
}

int photon_crc64ecma_fold_parts_n(const uint64_t* d_crc, const uint64_t* d_len, const uint64_t* d_obj_start,
                                  uint64_t nobj, uint64_t nparts, uint64_t seed0, const uint64_t* d_seeds,
                                  uint64_t* d_out, uint64_t* d_total, void* stream) {
    return fold_parts_n<Crc64>(d_crc, d_len, d_obj_start, nobj, nparts, seed0, d_seeds, d_out, d_total, stream);
}

// tuning.h, bench only: what a caller did before fold_parts_n existed.
int photon_crc_util_fold_on_host(int crc64, const void* d_crc, const uint64_t* h_len, const uint64_t* h_obj_start,
                                 uint64_t nobj, uint64_t nparts, uint64_t seed, void* h_out, void* stream) {
    if (!d_crc || !h_len || !h_obj_start || !h_out) return fail(-EINVAL, "null argument");
    if (int rc = photon_crc_stream_sync(stream)) return rc;
    const size_t w = crc64 ? 8 : 4;
    std::vector<uint8_t> h(nparts * w);
    hipError_t e = hipMemcpy(h.data(), d_crc, nparts * w, hipMemcpyDeviceToHost);
    if (e != hipSuccess) return hip_fail(e, "hipMemcpy");
    for (uint64_t m = 0; m < nobj; ++m) {
        if (crc64) {
            const uint64_t* c = reinterpret_cast<const uint64_t*>(h.data());
            uint64_t acc = seed;
            for (uint64_t s = h_obj_start[m]; s < h_obj_start[m + 1]; ++s)
                acc = crc64ecma_combine(acc, c[s], (uint32_t)h_len[s]);
            static_cast<uint64_t*>(h_out)[m] = acc;
        } else {
            const uint32_t* c = reinterpret_cast<const uint32_t*>(h.data());
            uint32_t acc = (uint32_t)seed;
            for (uint64_t s = h_obj_start[m]; s < h_obj_start[m + 1]; ++s)
                acc = crc32c_combine(acc, c[s], (uint32_t)h_len[s]);
            static_cast<uint32_t*>(h_out)[m] = acc;
        }
    }
    return 0;
}

// tuning.h: the kernels' per-thread and combine steps (fold_parts.h) on the host.
int photon_crc_test_fold_parts(int crc64, const void* crc, const uint64_t* len, uint64_t count, uint64_t seed,
                               uint32_t nthreads, uint64_t* result, uint64_t* total) {
    if (!result || !nthreads || ((!crc || !len) && count)) return fail(-EINVAL, "null argument or no threads");
    if (crc64)
        *result = fold_replay<Gf64>(static_cast<const uint64_t*>(crc), len, count, seed, nthreads,
                                    pow_table<Crc64>().x8pow2, total);
    else
        *result = fold_replay<Gf32>(static_cast<const uint32_t*>(crc), len, count, (uint32_t)seed, nthreads,
                                    pow_table<Crc32c>().x8pow2, total);
    return 0;
}

int photon_crc32c_overwrite_batch_strided(const void* src_base, uint64_t src_stride, void* d_dst_base,
                                          uint64_t dst_stride, uint64_t nbytes, uint64_t count, uint32_t* d_delta,
                                          void* stream) {
    return overwrite_batch_strided<Crc32c>(src_base, src_stride, d_dst_base, dst_stride, nbytes, count, d_delta, stream);
}

int photon_crc32c_overwrite_batch_iov(const photon_crc_iovec* d_src, void* const* d_dst, uint64_t count,
                                      uint32_t* d_delta, void* stream) {
    return overwrite_batch_iov<Crc32c>(d_src, d_dst, count, d_delta, stream);
}

int photon_crc64ecma_overwrite_batch_strided(const void* src_base, uint64_t src_stride, void* d_dst_base,
                                             uint64_t dst_stride, uint64_t nbytes, uint64_t count, uint64_t* d_delta,
                                             void* stream) {
    return overwrite_batch_strided<Crc64>(src_base, src_stride, d_dst_base, dst_stride, nbytes, count, d_delta, stream);
}

int photon_crc64ecma_overwrite_batch_iov(const photon_crc_iovec* d_src, void* const* d_dst, uint64_t count,
                                         uint64_t* d_delta, void* stream) {
    return overwrite_batch_iov<Crc64>(d_src, d_dst, count, d_delta, stream);
}

int photon_crc32c_patch_n(const uint32_t* d_delta, const uint64_t* d_tail, uint64_t nwrites,
                          const uint64_t* d_tgt_start, uint64_t ntgt, const uint32_t* d_crc_in, uint32_t* d_crc_out,
                          void* stream) {
    return patch_n<Crc32c>(d_delta, d_tail, nwrites, d_tgt_start, ntgt, d_crc_in, d_crc_out, stream);
}

int photon_crc64ecma_patch_n(const uint64_t* d_delta, const uint64_t* d_tail, uint64_t nwrites,
                             const uint64_t* d_tgt_start, uint64_t ntgt, const uint64_t* d_crc_in, uint64_t* d_crc_out,
                             void* stream) {
    return patch_n<Crc64>(d_delta, d_tail, nwrites, d_tgt_start, ntgt, d_crc_in, d_crc_out, stream);
}

// tuning.h: the patch kernel's steps (patch_crc.h) on the host.
int photon_crc_test_patch(int crc64, const void* delta, const uint64_t* tail, uint64_t nwrites,
                          const uint64_t* tgt_start, uint64_t ntgt, const void* crc_in, void* crc_out,
                          uint32_t nthreads) {
    if (!ntgt) return 0;
    if (!crc_in || !crc_out || !nthreads || ((!delta || !tail) && nwrites) || (!tgt_start && ntgt != nwrites))
        return fail(-EINVAL, "null argument, no threads, or a null tgt_start with ntgt != nwrites");
    if (crc64)
        patch_replay<Gf64>(static_cast<const uint64_t*>(delta), tail, nwrites, tgt_start, ntgt,
                           static_cast<const uint64_t*>(crc_in), static_cast<uint64_t*>(crc_out), nthreads,
                           pow_table<Crc64>().x8pow2);
    else
        patch_replay<Gf32>(static_cast<const uint32_t*>(delta), tail, nwrites, tgt_start, ntgt,
                           static_cast<const uint32_t*>(crc_in), static_cast<uint32_t*>(crc_out), nthreads,
                           pow_table<Crc32c>().x8pow2);
    return 0;
}

int photon_crc32c_xor_batch_strided(const void* src_base, uint64_t stripe_stride, uint64_t block_stride, uint32_t k,
                                    void* d_dst_base, uint64_t dst_stride, uint64_t nbytes, uint64_t count,
                                    uint32_t seed0, const uint32_t* d_seeds, uint32_t* d_out, void* stream) {
    return xor_batch_strided<Crc32c>(src_base, stripe_stride, block_stride, k, d_dst_base, dst_stride, nbytes, count,
                                     seed0, d_seeds, d_out, stream);
}

int photon_crc32c_xor_batch_ptr(const void* const* d_src, uint32_t k, const photon_crc_iovec* d_dst, uint64_t count,
                                uint32_t seed0, const uint32_t* d_seeds, uint32_t* d_out, void* stream) {
    return xor_batch_ptr<Crc32c>(d_src, k, d_dst, count, seed0, d_seeds, d_out, stream);
}

int photon_crc64ecma_xor_batch_strided(const void* src_base, uint64_t stripe_stride, uint64_t block_stride, uint32_t k,
                                       void* d_dst_base, uint64_t dst_stride, uint64_t nbytes, uint64_t count,
                                       uint64_t seed0, const uint64_t* d_seeds, uint64_t* d_out, void* stream) {
    return xor_batch_strided<Crc64>(src_base, stripe_stride, block_stride, k, d_dst_base, dst_stride, nbytes, count,
                                    seed0, d_seeds, d_out, stream);
}

int photon_crc64ecma_xor_batch_ptr(const void* const* d_src, uint32_t k, const photon_crc_iovec* d_dst,
                                   uint64_t count, uint64_t seed0, const uint64_t* d_seeds, uint64_t* d_out,
                                   void* stream) {
    return xor_batch_ptr<Crc64>(d_src, k, d_dst, count, seed0, d_seeds, d_out, stream);
}

int photon_crc32c_xor_expect_n(const uint32_t* d_crc, uint64_t ncrc, const uint64_t* d_grp_start, uint32_t k,
                               const uint64_t* d_len, uint64_t nbytes, uint64_t count, uint32_t seed,
                               uint32_t* d_want, void* stream) {
    return xor_expect_n<Crc32c>(d_crc, ncrc, d_grp_start, k, d_len, nbytes, count, seed, d_want, stream);
}

int photon_crc64ecma_xor_expect_n(const uint64_t* d_crc, uint64_t ncrc, const uint64_t* d_grp_start, uint32_t k,
                                  const uint64_t* d_len, uint64_t nbytes, uint64_t count, uint64_t seed,
                                  uint64_t* d_want, void* stream) {
    return xor_expect_n<Crc64>(d_crc, ncrc, d_grp_start, k, d_len, nbytes, count, seed, d_want, stream);
}

// tuning.h: the expect kernel's per-stripe step (xor_expect.h) on the host.
int photon_crc_test_xor_expect(int crc64, const void* crc, uint64_t ncrc, const uint64_t* grp_start, uint32_t k,
                               const uint64_t* len, uint64_t nbytes, uint64_t count, uint64_t seed, void* want) {
    if (!count) return 0;
    if (!xor_expect_args_ok(crc, ncrc, grp_start, k, want)) return fail(-EINVAL, kXorExpectArgs);
    if (crc64)
        xor_expect_replay<Gf64>(static_cast<const uint64_t*>(crc), ncrc, grp_start, k, len, nbytes, count, seed,
                                xor_expect_inv<Crc64>(), static_cast<uint64_t*>(want), pow_table<Crc64>().x8pow2);
    else
        xor_expect_replay<Gf32>(static_cast<const uint32_t*>(crc), ncrc, grp_start, k, len, nbytes, count,
                                (uint32_t)seed, xor_expect_inv<Crc32c>(), static_cast<uint32_t*>(want),
                                pow_table<Crc32c>().x8pow2);
    return 0;
}

// tuning.h: the stripe kernels' build constants.
int photon_crc_xor_geometry(int* in_flight, int* rows_per_step, int* rows_per_step64, int* max_sources) {
    if (in_flight) *in_flight = kXorInFlight;
    if (rows_per_step) *rows_per_step = PCRC_XOR_ROWS;
    if (rows_per_step64) *rows_per_step64 = PCRC_XOR_ROWS64;
    if (max_sources) *max_sources = (int)kXorMaxSources;
    return 0;
}

uint64_t photon_crc_scan_work_bytes(uint64_t nparts) {
    const uint64_t words = scan_work_words(nparts, scan_tile_now());
    return words == kScanNone ? ~0ull : words * 8;
}

int photon_crc32c_scan_parts_n(const uint32_t* d_crc, const uint64_t* d_len, const uint64_t* d_obj_start,
                               uint64_t nobj, uint64_t nparts, uint32_t seed0, const uint32_t* d_seeds,
                               uint32_t* d_run, uint64_t* d_end, void* d_work, uint64_t work_bytes, void* stream) {
    return scan_parts_n<Crc32c>(d_crc, d_len, d_obj_start, nobj, nparts, seed0, d_seeds, d_run, d_end, d_work,
                                work_bytes, stream);
}

int photon_crc64ecma_scan_parts_n(const uint64_t* d_crc, const uint64_t* d_len, const uint64_t* d_obj_start,
                                  uint64_t nobj, uint64_t nparts, uint64_t seed0, const uint64_t* d_seeds,
                                  uint64_t* d_run, uint64_t* d_end, void* d_work, uint64_t work_bytes, void* stream) {
    return scan_parts_n<Crc64>(d_crc, d_len, d_obj_start, nobj, nparts, seed0, d_seeds, d_run, d_end, d_work,
                               work_bytes, stream);
}

int photon_crc_set_scan_tile(uint32_t entries) {
    if (entries && !scan_tile_ok(entries))
        return fail(-EINVAL, "scan tile: 0 (the default) or a power of two from 64 to 65536");
    g_scan_tile.store(entries, std::memory_order_relaxed);
    return 0;
}

void photon_crc_test_scan_geometry(uint64_t out[3]) {
    out[0] = scan_tile_now();
    out[1] = kScanChunk;
    out[2] = kScanMaxGrid;
}

// tuning.h: the kernels' three steps (scan_parts.h) on the host.
int photon_crc_test_scan_parts(int crc64, const void* crc, const uint64_t* len, const uint64_t* obj_start,
                               uint64_t nobj, uint64_t nparts, uint64_t seed0, const void* seeds, uint32_t tile,
                               uint32_t nthreads, void* run, uint64_t* end) {
    if (!nobj || !nparts) return 0;
    if (!crc || !len || !run || !nthreads || (!obj_start && nobj != 1))
        return fail(-EINVAL, "null argument or no threads");
    if (!scan_tile_ok(tile) || nparts > kScanMaxParts) return fail(-EINVAL, "bad tile or too many parts");
    std::vector<uint64_t> work(scan_work_words(nparts, tile), 0xA5A5A5A5A5A5A5A5ull);
    if (crc64) {
        const ScanIn<uint64_t> in = {static_cast<const uint64_t*>(crc), len, obj_start, nobj, nparts, seed0,
                                     static_cast<const uint64_t*>(seeds)};
        scan_replay<Gf64>(in, tile, nthreads, pow_table<Crc64>().x8pow2, work.data(), static_cast<uint64_t*>(run), end);
    } else {
        const ScanIn<uint32_t> in = {static_cast<const uint32_t*>(crc), len, obj_start, nobj, nparts, (uint32_t)seed0,
                                     static_cast<const uint32_t*>(seeds)};
        scan_replay<Gf32>(in, tile, nthreads, pow_table<Crc32c>().x8pow2, work.data(), static_cast<uint32_t*>(run), end);
    }
    return 0;
}

// tuning.h, bench only: what a caller did before the scan calls existed.
int photon_crc_util_scan_on_host(int crc64, const void* d_crc, void* h_crc, const uint64_t* h_len,
                                 const uint64_t* h_obj_start, uint64_t nobj, uint64_t nparts, uint64_t seed,
                                 void* h_run, void* d_run, void* stream) {
    if (!d_crc || !h_crc || !h_len || !h_obj_start || !h_run || !d_run) return fail(-EINVAL, "null argument");
    if (int rc = photon_crc_stream_sync(stream)) return rc;
    const size_t w = crc64 ? 8 : 4;
    hipError_t e = hipMemcpy(h_crc, d_crc, nparts * w, hipMemcpyDeviceToHost);
    if (e != hipSuccess) return hip_fail(e, "hipMemcpy");
    for (uint64_t m = 0; m < nobj; ++m) {
        if (crc64) {
            const uint64_t* c = static_cast<const uint64_t*>(h_crc);
            uint64_t acc = seed;
            for (uint64_t s = h_obj_start[m]; s < h_obj_start[m + 1]; ++s)
                static_cast<uint64_t*>(h_run)[s] = acc = crc64ecma_combine(acc, c[s], (uint32_t)h_len[s]);
        } else {
            const uint32_t* c = static_cast<const uint32_t*>(h_crc);
            uint32_t acc = (uint32_t)seed;
            for (uint64_t s = h_obj_start[m]; s < h_obj_start[m + 1]; ++s)
                static_cast<uint32_t*>(h_run)[s] = acc = crc32c_combine(acc, c[s], (uint32_t)h_len[s]);
        }
    }
    e = hipMemcpy(d_run, h_run, nparts * w, hipMemcpyHostToDevice);
    return e == hipSuccess ? 0 : hip_fail(e, "hipMemcpy");
}

uint64_t photon_crc_verify_work_bytes(uint64_t count) {
    const uint64_t words = verify_work_words(count, verify_tile_now());
    return words == kVerifyNone ? ~0ull : words * 8;
}

int photon_crc32c_verify_n(const uint32_t* d_crc, const void* d_expected, uint64_t expected_stride, uint64_t count,
                           photon_crc_verify_report* d_report, uint64_t* d_bad_idx, uint64_t bad_cap, void* d_work,
                           uint64_t work_bytes, void* stream) {
    return verify_n<Crc32c>(d_crc, d_expected, expected_stride, nullptr, false, count, d_report, d_bad_idx, bad_cap,
                            d_work, work_bytes, stream);
}

int photon_crc64ecma_verify_n(const uint64_t* d_crc, const void* d_expected, uint64_t expected_stride,
                              uint64_t count, photon_crc_verify_report* d_report, uint64_t* d_bad_idx,
                              uint64_t bad_cap, void* d_work, uint64_t work_bytes, void* stream) {
    return verify_n<Crc64>(d_crc, d_expected, expected_stride, nullptr, false, count, d_report, d_bad_idx, bad_cap,
                           d_work, work_bytes, stream);
}

int photon_crc32c_verify_ptr_n(const uint32_t* d_crc, const void* const* d_expected_ptr, uint64_t count,
                               photon_crc_verify_report* d_report, uint64_t* d_bad_idx, uint64_t bad_cap,
                               void* d_work, uint64_t work_bytes, void* stream) {
    return verify_n<Crc32c>(d_crc, nullptr, 0, d_expected_ptr, true, count, d_report, d_bad_idx, bad_cap, d_work,
                            work_bytes, stream);
}

int photon_crc64ecma_verify_ptr_n(const uint64_t* d_crc, const void* const* d_expected_ptr, uint64_t count,
                                  photon_crc_verify_report* d_report, uint64_t* d_bad_idx, uint64_t bad_cap,
                                  void* d_work, uint64_t work_bytes, void* stream) {
    return verify_n<Crc64>(d_crc, nullptr, 0, d_expected_ptr, true, count, d_report, d_bad_idx, bad_cap, d_work,
                           work_bytes, stream);
}

int photon_crc32c_stamp_n(const uint32_t* d_crc, uint64_t count, void* d_dst, uint64_t dst_stride, void* stream) {
    return stamp_n<Crc32c>(d_crc, count, d_dst, dst_stride, nullptr, false, stream);
}

int photon_crc64ecma_stamp_n(const uint64_t* d_crc, uint64_t count, void* d_dst, uint64_t dst_stride, void* stream) {
    return stamp_n<Crc64>(d_crc, count, d_dst, dst_stride, nullptr, false, stream);
}

int photon_crc32c_stamp_ptr_n(const uint32_t* d_crc, uint64_t count, void* const* d_dst_ptr, void* stream) {
    return stamp_n<Crc32c>(d_crc, count, nullptr, 0, d_dst_ptr, true, stream);
}

int photon_crc64ecma_stamp_ptr_n(const uint64_t* d_crc, uint64_t count, void* const* d_dst_ptr, void* stream) {
    return stamp_n<Crc64>(d_crc, count, nullptr, 0, d_dst_ptr, true, stream);
}

int photon_crc_set_verify_tile(uint32_t entries) {
    if (entries && !verify_tile_ok(entries))
        return fail(-EINVAL, "verify tile: 0 (the default) or a power of two from 64 to 65536");
    g_verify_tile.store(entries, std::memory_order_relaxed);
    return 0;
}

// tuning.h: the kernels' three steps (verify_scan.h) on the host.
int photon_crc_test_verify(int crc64, const void* crc, const void* expected, uint64_t expected_stride,
                           const void* const* expected_ptr, uint64_t count, uint32_t tile, uint64_t bad_cap,
                           uint64_t report[4], uint64_t* bad_idx) {
    if (!count || !crc || (!expected && !expected_ptr) || !report || (!bad_idx && bad_cap))
        return fail(-EINVAL, "null argument or no entries");
    if (!verify_tile_ok(tile) || count > kVerifyMaxCount) return fail(-EINVAL, "bad tile or too many entries");
    std::vector<uint64_t> work(verify_work_words(count, tile), 0xA5A5A5A5A5A5A5A5ull);
    if (crc64)
        verify_replay<uint64_t>(static_cast<const uint64_t*>(crc), expected, expected_stride, expected_ptr, count, tile,
                                bad_cap, work.data(), report, bad_idx);
    else
        verify_replay<uint32_t>(static_cast<const uint32_t*>(crc), expected, expected_stride, expected_ptr, count, tile,
                                bad_cap, work.data(), report, bad_idx);
    return 0;
}

// tuning.h, bench only: what a caller did before the verify calls existed.
int photon_crc_util_verify_on_host(int crc64, const void* d_crc, void* h_crc, const void* h_expected, uint64_t count,
                                   uint64_t report[4], uint64_t* h_bad_idx, uint64_t bad_cap, void* stream) {
    if (!d_crc || !h_crc || !h_expected || !report || (!h_bad_idx && bad_cap)) return fail(-EINVAL, "null argument");
    if (int rc = photon_crc_stream_sync(stream)) return rc;
    const size_t w = crc64 ? 8 : 4;
    const hipError_t e = hipMemcpy(h_crc, d_crc, count * w, hipMemcpyDeviceToHost);
    if (e != hipSuccess) return hip_fail(e, "hipMemcpy");
    uint64_t nbad = 0, first = ~0ull;
    auto loop = [&](auto* c, auto* x) {
        for (uint64_t i = 0; i < count; ++i) {
            if (c[i] == x[i]) continue;
            if (!nbad) first = i;
            if (nbad < bad_cap) h_bad_idx[nbad] = i;
            ++nbad;
        }
    };
    if (crc64) loop(static_cast<const uint64_t*>(h_crc), static_cast<const uint64_t*>(h_expected));
    else loop(static_cast<const uint32_t*>(h_crc), static_cast<const uint32_t*>(h_expected));
    report[0] = nbad;
    report[1] = first;
    report[2] = nbad < bad_cap ? nbad : bad_cap;
    report[3] = count;
    return 0;
}

int photon_crc32c_copy_parts_n(const photon_crc_iovec* d_src, void* const* d_dst, uint64_t nparts,
                               uint64_t max_part_bytes, uint32_t seed0, const uint32_t* d_seeds, uint32_t* d_out,
                               void* d_work, uint64_t work_bytes, void* stream) {
    return parts_n<Crc32c, true>(d_src, d_dst, nparts, max_part_bytes, seed0, d_seeds, d_out, d_work, work_bytes,
                                 stream);
}

int photon_crc64ecma_copy_parts_n(const photon_crc_iovec* d_src, void* const* d_dst, uint64_t nparts,
                                  uint64_t max_part_bytes, uint64_t seed0, const uint64_t* d_seeds, uint64_t* d_out,
                                  void* d_work, uint64_t work_bytes, void* stream) {
    return parts_n<Crc64, true>(d_src, d_dst, nparts, max_part_bytes, seed0, d_seeds, d_out, d_work, work_bytes,
                                stream);
}

int photon_crc32c_batch_parts_n(const photon_crc_iovec* d_iov, uint64_t nparts, uint64_t max_part_bytes,
                                uint32_t seed0, const uint32_t* d_seeds, uint32_t* d_out, void* d_work,
                                uint64_t work_bytes, void* stream) {
    return parts_n<Crc32c, false>(d_iov, nullptr, nparts, max_part_bytes, seed0, d_seeds, d_out, d_work, work_bytes,
                                  stream);
}

int photon_crc64ecma_batch_parts_n(const photon_crc_iovec* d_iov, uint64_t nparts, uint64_t max_part_bytes,
                                   uint64_t seed0, const uint64_t* d_seeds, uint64_t* d_out, void* d_work,
                                   uint64_t work_bytes, void* stream) {
    return parts_n<Crc64, false>(d_iov, nullptr, nparts, max_part_bytes, seed0, d_seeds, d_out, d_work, work_bytes,
                                 stream);
}

uint64_t photon_crc_parts_work_bytes(uint64_t nparts, uint64_t max_part_bytes, int crc64) {
    PartsPlan pl;
    if (!parts_plan(nparts, max_part_bytes, parts_piece_now(), &pl)) return ~0ull;
    return pl.ntasks * (crc64 ? sizeof(uint64_t) : sizeof(uint32_t));
}

int photon_crc_set_host_stage_bytes(uint64_t bytes) {
    if (!stage_span_valid(bytes))
        return fail(-EINVAL, "host stage bytes: 0 (default) or a multiple of 256 from 64 KiB to 256 MiB");
    g_host_stage.store(bytes, std::memory_order_relaxed);
    return 0;
}

int photon_crc_set_parts_piece(uint64_t bytes) {
    if (bytes % kPartsAlign || bytes > kPartsMaxPiece)
        return fail(-EINVAL, "parts piece: 0 (automatic) or a multiple of 4096 up to 1 GiB");
    g_parts_piece.store(bytes, std::memory_order_relaxed);
    return 0;
}

int photon_crc_util_parts_fold(int crc64, const void* d_iov, uint64_t nparts, uint64_t max_part_bytes,
                               uint64_t seed0, const void* d_seeds, void* d_out, const void* d_work, void* stream) {
    if (!nparts) return 0;
    if (!d_iov || !d_out || !d_work) return fail(-EINVAL, "null argument");
    const photon_crc_iovec* d_src = static_cast<const photon_crc_iovec*>(d_iov);
    PartsPlan pl;
    if (!parts_plan(nparts, max_part_bytes, parts_piece_now(), &pl)) return fail(-EINVAL, "too many tasks");
    int cus = 0;
    const int dev = current_device(&cus);
    if (dev < 0) return dev;
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (crc64)
        launch_parts_fold<Crc64>(d_src, nparts, pl, static_cast<const uint64_t*>(d_work), seed0,
                                 static_cast<const uint64_t*>(d_seeds), static_cast<uint64_t*>(d_out), st);
    else
        launch_parts_fold<Crc32c>(d_src, nparts, pl, static_cast<const uint32_t*>(d_work), (uint32_t)seed0,
                                  static_cast<const uint32_t*>(d_seeds), static_cast<uint32_t*>(d_out), st);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : hip_fail(e, crc64 ? Crc64::kPartsFoldLaunch : Crc32c::kPartsFoldLaunch);
}

int photon_crc_test_parts_plan(uint64_t addr, uint64_t len, uint64_t max_part_bytes, uint64_t piece, uint64_t* out,
                               int cap) {
    if (!out || cap < 2 || piece % kPartsAlign || piece > kPartsMaxPiece) return fail(-EINVAL, "bad plan arguments");
    PartsPlan pl;
    if (!parts_plan(1, max_part_bytes, piece ? piece : parts_piece_now(), &pl)) return fail(-EINVAL, "too many tasks");
    const uint64_t n = len < pl.max_bytes ? len : pl.max_bytes;
    int k = 2;
    uint64_t count = 0;
    // every slot of the part, as the piece kernel walks them: the empty ones are left out
    for (uint64_t j = 0; j < pl.per_part; ++j) {
        const PartsPiece pc = parts_piece(addr, n, pl.piece, j);
        if (!pc.len) continue;
        if (k + 2 > cap) return fail(-EINVAL, "short output");
        out[k++] = pc.off;
        out[k++] = pc.len;
        ++count;
    }
    if (count != parts_count(addr, n, pl.piece)) return fail(-EIO, "parts plan: piece count mismatch");
    out[0] = pl.per_part;
    out[1] = count;
    return k;
}

int photon_crc32c_copy_parts_packed_n(const photon_crc_iovec* d_src, void* const* d_dst, uint64_t nparts,
                                      uint64_t max_part_bytes, uint64_t max_total_bytes, uint32_t seed0,
                                      const uint32_t* d_seeds, uint32_t* d_out, uint64_t* d_report, void* d_work,
                                      uint64_t work_bytes, void* stream) {
    return parts_packed_n<Crc32c, true>(d_src, d_dst, nparts, max_part_bytes, max_total_bytes, seed0, d_seeds, d_out,
                                        d_report, d_work, work_bytes, stream);
}

int photon_crc64ecma_copy_parts_packed_n(const photon_crc_iovec* d_src, void* const* d_dst, uint64_t nparts,
                                         uint64_t max_part_bytes, uint64_t max_total_bytes, uint64_t seed0,
                                         const uint64_t* d_seeds, uint64_t* d_out, uint64_t* d_report, void* d_work,
                                         uint64_t work_bytes, void* stream) {
    return parts_packed_n<Crc64, true>(d_src, d_dst, nparts, max_part_bytes, max_total_bytes, seed0, d_seeds, d_out,
                                       d_report, d_work, work_bytes, stream);
}

int photon_crc32c_batch_parts_packed_n(const photon_crc_iovec* d_iov, uint64_t nparts, uint64_t max_part_bytes,
                                       uint64_t max_total_bytes, uint32_t seed0, const uint32_t* d_seeds,
                                       uint32_t* d_out, uint64_t* d_report, void* d_work, uint64_t work_bytes,
                                       void* stream) {
    return parts_packed_n<Crc32c, false>(d_iov, nullptr, nparts, max_part_bytes, max_total_bytes, seed0, d_seeds,
                                         d_out, d_report, d_work, work_bytes, stream);
}

int photon_crc64ecma_batch_parts_packed_n(const photon_crc_iovec* d_iov, uint64_t nparts, uint64_t max_part_bytes,
                                          uint64_t max_total_bytes, uint64_t seed0, const uint64_t* d_seeds,
                                          uint64_t* d_out, uint64_t* d_report, void* d_work, uint64_t work_bytes,
                                          void* stream) {
    return parts_packed_n<Crc64, false>(d_iov, nullptr, nparts, max_part_bytes, max_total_bytes, seed0, d_seeds,
                                        d_out, d_report, d_work, work_bytes, stream);
}

uint64_t photon_crc_parts_packed_work_bytes(uint64_t nparts, uint64_t max_total_bytes, int crc64) {
    if (!nparts) return 0;
    PackedPlan pl;
    if (packed_plan(nparts, 0, max_total_bytes, parts_piece_now(), crc64 ? 8 : 4, &pl)) return ~0ull;
    return pl.at.bytes;
}

int photon_crc_util_parts_packed_plan(int crc64, const void* d_iov, uint64_t nparts, uint64_t max_part_bytes,
                                      uint64_t max_total_bytes, uint64_t* d_report, void* d_work, void* stream) {
    if (!nparts) return 0;
    if (!d_iov || !d_report || !d_work || ((uintptr_t)d_work & 7u)) return fail(-EINVAL, "null or misaligned argument");
    PackedPlan pl;
    if (packed_plan(nparts, max_part_bytes, max_total_bytes, parts_piece_now(), crc64 ? 8 : 4, &pl))
        return fail(-EINVAL, "too many parts or piece slots");
    int cus = 0;
    const int dev = current_device(&cus);
    if (dev < 0) return dev;
    char* work = static_cast<char*>(d_work);
    int rc = 0;
    launch_packed_plan(static_cast<const photon_crc_iovec*>(d_iov), nparts, pl,
                       reinterpret_cast<uint64_t*>(work + pl.at.tiles), reinterpret_cast<uint64_t*>(work + pl.at.first),
                       reinterpret_cast<uint32_t*>(work + pl.at.owner), d_report, static_cast<hipStream_t>(stream),
                       [&](const char* what) {
                           const hipError_t e = hipGetLastError();
                           if (e != hipSuccess) rc = hip_fail(e, "parts_packed", what);
                           return e == hipSuccess;
                       });
    return rc;
}

int photon_crc_test_parts_packed_plan(const uint64_t* addr, const uint64_t* len, uint64_t nparts,
                                      uint64_t max_part_bytes, uint64_t max_total_bytes, uint64_t piece,
                                      uint64_t* first, uint64_t* report, uint64_t* tasks, uint64_t task_cap) {
    if (!addr || !len || !nparts || !first || !report || (!tasks && task_cap) || piece % kPartsAlign ||
        piece > kPartsMaxPiece)
        return fail(-EINVAL, "bad packed plan arguments");
    PackedPlan pl;
    if (packed_plan(nparts, max_part_bytes, max_total_bytes, piece ? piece : parts_piece_now(), 4, &pl))
        return fail(-EINVAL, "too many parts or piece slots");
    // the workspace as a call has it: exactly its size, never cleared
    std::vector<uint64_t> work((pl.at.bytes + 7) / 8, 0x5A5A5A5A5A5A5A5Aull);
    uint8_t* w = reinterpret_cast<uint8_t*>(work.data());
    packed_replay(addr, len, nparts, pl.max_bytes, pl.piece, pl.slots, 4, w, report);
    const uint64_t* f = reinterpret_cast<const uint64_t*>(w + pl.at.first);
    const uint32_t* owner = reinterpret_cast<const uint32_t*>(w + pl.at.owner);
    for (uint64_t i = 0; i <= nparts; ++i) first[i] = f[i];
    const uint64_t bound = packed_bound(f[nparts], pl.slots);
    if (bound > task_cap) return fail(-EINVAL, "short output");
    for (uint64_t t = 0; t < bound; ++t) {  // as parts_packed_task derives it
        const uint64_t i = packed_owner_clamp(owner[t], nparts);
        const uint64_t n = len[i] < pl.max_bytes ? len[i] : pl.max_bytes;
        const PartsPiece pc = packed_piece(addr[i], n, pl.piece, f[i], t);
        tasks[3 * t] = i;
        tasks[3 * t + 1] = pc.off;
        tasks[3 * t + 2] = pc.len;
    }
    return 0;
}

int photon_crc32c_trim_batch(const photon_crc_component* d_all, const photon_crc_component* d_prefix,
                             const photon_crc_component* d_suffix, uint64_t count, uint32_t* d_out,
                             uint32_t* d_nerr, void* stream) {
    return trim_batch<Crc32c>(d_all, d_prefix, d_suffix, count, d_out, d_nerr, stream);
}

int photon_crc32c_extend_device(const void* d_data, uint64_t nbytes, uint32_t seed, uint32_t* d_out, void* stream) {
    return extend_device<Crc32c>(d_data, nbytes, seed, d_out, stream);
}

int photon_crc32c_copy_extend_device(const void* src, void* d_dst, uint64_t nbytes, uint32_t seed, uint32_t* d_out,
                                     void* stream) {
    return copy_extend_device<Crc32c>(src, d_dst, nbytes, seed, d_out, stream);
}
}  // extern "C"

namespace pcrc {
namespace {

// photon_crc32c_extend_spans / photon_crc64ecma_extend_spans: every span's
// CRC (seed 0) on its own device, the kernels of all devices enqueued before
// any wait, then the host fold acc = acc * x^(8 len) ^ crc (crc.cpp:393-405).
template <typename T, typename Launch, typename Shift>
int extend_spans(const photon_crc_span* spans, int nspans, T seed, T* h_result, Launch launch, Shift shift) {
    if (nspans < 0 || (nspans && !spans) || !h_result) return fail(-EINVAL, "bad span list or result");
    if (nspans == 0) {  // the empty buffer: its CRC is the seed
        *h_result = seed;
        return 0;
    }
    std::vector<void*> outs(nspans, nullptr);
    std::vector<T> crcs(nspans, 0);
    HipRT rt;
    // Every span's kernel enqueued on its own device before any wait...
    int issued = 0;
    int rc = run_on_devices(
        rt, nspans, [&](int i) { return spans[i].device; },
        [&](int i) {
            const photon_crc_span& sp = spans[i];
            if (!sp.d_data && sp.nbytes) return fail(-EINVAL, "null span with bytes");
            if (int r = scratch_alloc(&outs[i], sizeof(T), nullptr)) return r;
            return launch(sp.d_data, sp.nbytes, static_cast<T*>(outs[i]));
        },
        &issued);
    // ...then collected (and every lease returned, even after a failure --
    // a device that refuses the switch included: the later spans' leases are
    // still returned on their own devices), each on its device.
    int first = 0;  // the first collection error; the loop goes on so that every lease is returned
    const int set_rc = run_on_every_device(
        rt, issued, [&](int i) { return spans[i].device; },
        [&](int i) {
            if (!outs[i]) return 0;
            if (!rc && !first) {
                const hipError_t e = hipMemcpy(&crcs[i], outs[i], sizeof(T), hipMemcpyDeviceToHost);
                if (e != hipSuccess) first = hip_fail(e, "hipMemcpy(span CRC)");
            }
            const int frc = scratch_free(outs[i], nullptr);
            if (!first) first = frc;
            return 0;
        });
    if (!rc) rc = first ? first : set_rc;
    if (rc) return rc;
    T acc = seed;
    for (int i = 0; i < nspans; ++i) acc = shift(acc, spans[i].nbytes) ^ crcs[i];
    *h_result = acc;
    return 0;
}

}  // namespace
}  // namespace pcrc

extern "C" {

int photon_crc32c_extend_spans(const photon_crc_span* spans, int nspans, uint32_t seed, uint32_t* h_result) {
    return extend_spans<uint32_t>(
        spans, nspans, seed, h_result,
        [](const void* p, uint64_t n, uint32_t* o) { return photon_crc32c_extend_device(p, n, 0, o, nullptr); },
        [](uint32_t acc, uint64_t n) { return acc ? shift_bytes(acc, n) : 0u; });
}

int photon_crc64ecma_extend_spans(const photon_crc_span* spans, int nspans, uint64_t seed, uint64_t* h_result) {
    return extend_spans<uint64_t>(
        spans, nspans, seed, h_result,
        [](const void* p, uint64_t n, uint64_t* o) { return photon_crc64ecma_extend_device(p, n, 0, o, nullptr); },
        [](uint64_t acc, uint64_t n) { return acc ? mulmod64(acc, xpow64(8 * n)) : 0ull; });
}

int64_t photon_crc_scratch_release(void) {
    std::lock_guard<std::mutex> lk(g_scr_mu);
    return scratch_trim_locked(true);
}

int photon_crc_util_read_stream(const void* d_base, uint64_t nbytes, uint32_t* d_sink, uint64_t sink_words,
                                void* stream) {
    if (!d_base || !d_sink || (reinterpret_cast<uintptr_t>(d_base) & 15)) return fail(-EINVAL, "bad arguments");
    int cus = 0;
    int dev = current_device(&cus);
    if (dev < 0) return dev;
    uint64_t grid = (uint64_t)cus;  // one persistent 16-wave workgroup per CU, as the batch kernels
    if (grid * kBlock > sink_words) grid = sink_words / kBlock;
    if (!grid) return fail(-EINVAL, "sink too small (need >= 1024 words)");
    hipLaunchKernelGGL(read_stream_kernel, dim3(grid), dim3(kBlock), 0, static_cast<hipStream_t>(stream),
                       static_cast<const uint8_t*>(d_base), nbytes, d_sink);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return hip_fail(e, "read_stream_kernel launch");
    return 0;
}

int photon_crc_util_fill_splitmix(void* d_base, uint64_t stride, uint64_t nbytes, uint64_t count,
                                  uint64_t seed_base, void* stream) {
    if (!count || !nbytes) return 0;
    if (!d_base) return fail(-EINVAL, "null buffer");
    int cus = 0;
    int dev = current_device(&cus);
    if (dev < 0) return dev;
    const uint64_t words = (nbytes + 7) / 8 * count;
    uint64_t grid = (words + 255) / 256;
    if (grid > (uint64_t)cus * 16) grid = (uint64_t)cus * 16;
    hipLaunchKernelGGL(fill_splitmix_kernel, dim3(grid), dim3(256), 0, static_cast<hipStream_t>(stream),
                       static_cast<uint8_t*>(d_base), stride, nbytes, count, seed_base);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return hip_fail(e, "fill_splitmix_kernel launch");
    return 0;
}

}  // extern "C"

// ------------------------------------------------------------ device dispatch
// photon_crc_set_device_dispatch: the drop-in dispatch pointers (crc.cpp:126-134)
// routed to the calls above when the data pointer is device memory.
namespace pcrc {
namespace {

std::mutex g_dispatch_mu;
std::atomic<int> g_dispatch_err{0};
std::atomic<bool> g_dispatch_on{false};  // written under g_dispatch_mu; read by heavy_mark

// The saved host engines (Crc32c::host_crc ..., Crc64::host_cseries), read by
// the routed wrappers.
template <typename F>
F host_engine(F* slot) {
    return __atomic_load_n(slot, __ATOMIC_RELAXED);
}

// Device owning `p`, or -1 for host / unregistered memory.
int device_of(const void* p) {
    if (!p) return -1;
    hipPointerAttribute_t attr;
    if (hipPointerGetAttributes(&attr, p) != hipSuccess) {
        (void)hipGetLastError();  // do not leave the probe's error for the caller
        return -1;
    }
    return attr.type == hipMemoryTypeDevice ? attr.device : -1;
}

struct DeviceScope {
    int prev = -1;
    explicit DeviceScope(int dev) {
        int cur = -1;
        if (hipGetDevice(&cur) == hipSuccess && cur != dev && hipSetDevice(dev) == hipSuccess) prev = cur;
    }
    ~DeviceScope() {
        if (prev >= 0) (void)hipSetDevice(prev);
    }
};

// A routed call that fails has no error channel in the reference signature,
// and the reference always computes (crc.cpp:114-117): never return a made-up
// value. The failure is reported loudly (stderr, counter, sticky flag, errno
// = EIO) and the bytes are copied to the host and checksummed by the host
// engine -- the same result the reference returns. If even that copy fails
// (the device is gone), there is no right answer to give: abort.
std::atomic<uint64_t> g_fallbacks{0};

void routed_failure(const char* what, int rc) {
    g_dispatch_err.store(1);
    g_fallbacks.fetch_add(1);
    fprintf(stderr, "photon_crc device dispatch: %s failed on the device (%d): %s; recomputing on the host\n", what,
            rc, g_err.c_str());
    errno = EIO;
}

[[noreturn]] void routed_abort(const char* what, hipError_t e) {
    fprintf(stderr, "photon_crc device dispatch: %s: device copy for the host recomputation failed: %s; aborting "
            "rather than returning a wrong checksum\n", what, hipGetErrorString(e));
    abort();
}

// Feed [p, p+n) of device memory through host memory in chunks.
template <typename F>
void for_host_chunks(const uint8_t* p, size_t n, const char* what, F f) {
    constexpr size_t kChunk = 16u << 20;
    std::vector<uint8_t> buf(n < kChunk ? n : kChunk);
    for (size_t off = 0; off < n; off += buf.size()) {
        const size_t k = n - off < buf.size() ? n - off : buf.size();
        hipError_t e = hipMemcpy(buf.data(), p + off, k, hipMemcpyDeviceToHost);
        if (e != hipSuccess) routed_abort(what, e);
        f(buf.data(), k);
    }
}

template <typename W>
typename W::T host_crc_of_device(const uint8_t* p, size_t n, typename W::T crc) {
    const auto eng = host_engine(&W::host_crc);
    for_host_chunks(p, n, W::kExtend, [&](const uint8_t* h, size_t k) { crc = eng(h, k, crc); });
    return crc;
}

// Routed calls run on a stream leased from a per-device pool of non-blocking
// streams (created on demand and kept), never on the null stream: a routed
// call does not serialise against the process's other blocking streams, and
// routed calls from many threads each get a stream of their own (VERDICT r3
// next #3). Each pooled stream carries kRoutedArea bytes of pinned, device-mapped
// host memory that a kernel writes its result into: the caller waits for
// the stream and reads the word(s), no D2H copy. A small buffer's CRC comes
// back as one word per workgroup of crc32c_small_kernel, XORed here: no
// cross-workgroup reduce on the device.
// Bytes of a routed stream's pinned result area: the small kernels' slots
// (CRC-64: 16 bytes per workgroup) or a long kernel's tagged words.
constexpr uint64_t kRoutedArea = 16 * kSmallWg > 512 ? 1024 : 512;
static_assert(16 * kSmallWg <= kRoutedArea, "routed result area");
struct RoutedStream {
    int dev;
    hipStream_t st;
    void* h;  // host address of the result area
    void* d;  // its device address
    uint32_t tag;  // last tag of a spin-waited call (crc32c_small_kernel slots)
};
std::mutex g_rs_mu;
std::vector<RoutedStream*> g_rs_free;

int routed_lease(int dev, RoutedStream** out) {
    {
        std::lock_guard<std::mutex> lk(g_rs_mu);
        for (size_t i = 0; i < g_rs_free.size(); ++i)
            if (g_rs_free[i]->dev == dev) {
                *out = g_rs_free[i];
                g_rs_free.erase(g_rs_free.begin() + (long)i);
                return 0;
            }
    }
    auto* r = new RoutedStream{dev, nullptr, nullptr, nullptr, 0};
    hipError_t e = hipStreamCreateWithFlags(&r->st, hipStreamNonBlocking);
    // coherent: the small kernel's system-scope tag stores reach the host directly
    if (e == hipSuccess)
        e = hipHostMalloc(&r->h, kRoutedArea, hipHostMallocMapped | hipHostMallocPortable | hipHostMallocCoherent);
    if (e == hipSuccess) memset(r->h, 0, kRoutedArea);
    if (e == hipSuccess) e = hipHostGetDevicePointer(&r->d, r->h, 0);
    if (e != hipSuccess) {
        if (r->h) (void)hipHostFree(r->h);
        if (r->st) (void)hipStreamDestroy(r->st);
        delete r;
        return hip_fail(e, "routed stream");
    }
    *out = r;
    return 0;
}

void routed_return(RoutedStream* r) {
    std::lock_guard<std::mutex> lk(g_rs_mu);
    g_rs_free.push_back(r);
}

// Run f(d_result, stream) on a leased routed stream and wait; the kernel's
// `bytes`-byte result lands in pinned memory and is copied to h_out.
template <typename F>
int routed_call(int dev, void* h_out, size_t bytes, F f) {
    RoutedStream* r = nullptr;
    if (int rc = routed_lease(dev, &r)) return rc;
    int rc = f(r->d, r->st);
    const hipError_t e = hipStreamSynchronize(r->st);  // also after a failed enqueue: nothing left running
    if (!rc && e != hipSuccess) rc = hip_fail(e, "hipStreamSynchronize(routed)");
    if (!rc) memcpy(h_out, r->h, bytes);
    routed_return(r);
    return rc;
}

// Run f(d_tmp, stream) with `bytes` of leased device scratch on a leased
// routed stream, copy `out_bytes` of it to `h_out`, and wait.
template <typename F>
int with_scratch(int dev, uint64_t bytes, void* h_out, uint64_t out_bytes, F f) {
    RoutedStream* r = nullptr;
    if (int rc = routed_lease(dev, &r)) return rc;
    void* tmp = nullptr;
    int rc = scratch_alloc(&tmp, bytes, r->st);
    hipError_t e;
    if (!rc) {
        rc = f(tmp, r->st);
        if (!rc) {
            e = hipMemcpyAsync(h_out, tmp, out_bytes, hipMemcpyDeviceToHost, r->st);
            if (e != hipSuccess) rc = hip_fail(e, "hipMemcpyAsync");
        }
        const int frc = scratch_free(tmp, r->st);
        if (!rc) rc = frc;
    }
    e = hipStreamSynchronize(r->st);
    if (!rc && e != hipSuccess) rc = hip_fail(e, "hipStreamSynchronize");
    routed_return(r);
    return rc;
}

// Collecting a routed call's result (crc32c.h:30-33 is synchronous). The
// kernels store their result words tagged, at system scope, into the routed
// stream's pinned area, and the caller polls the tags: a completion signal
// would add microseconds to a 5 µs kernel. The poll is bounded so that a
// routed call does not hold a Photon vCPU (rpc.cpp:379: coroutines share the
// thread, thread/thread.h:511-520) for the whole of a long kernel:
//   1. a call whose kernel is expected to run longer than the poll window
//      (its bytes at a nominal 6.5 GB/ms) first sleeps through 85 % of that
//      time (nanosleep with this thread's timer slack at 1 ns for the wait,
//      restored after: the default 50 µs slack would add that much latency);
//   2. then polls the tags with a pause between reads for at most the window
//      (g_routed_wait, default 40 µs);
//   3. then sleeps in 10 µs slices, reading the tags after each and asking
//      the stream for errors every 10th; a stream that finished (or failed)
//      without every tag returns its error.
// (hipEventSynchronize on a hipEventBlockingSync event kept the thread 100 %
// busy on ROCm 7.2, repo:profiles/r05d_bench_extend.json: it is not used.
// 1 GiB at buf+1, repo:profiles/r05e_bench_extend.json: pure spinning 172.0
// µs at 100 % of a core; 80 % sleep + 30 µs window 180.2 µs at 20.9 %; 10 µs
// slices only 178.0 µs at 12.7 %; 128 KiB 10.9-11.7 µs either way.)
// photon_crc_set_routed_wait (tuning.h) changes the window and step 1.
constexpr double kNominalBytesPerUs = 6.5e6;  // ~81 % of 8 TB/s: a long kernel's expected rate

inline void cpu_relax() {
#if defined(__x86_64__) && !defined(__HIP_DEVICE_COMPILE__)
    __builtin_ia32_pause();
#endif
}

// This thread's timer slack at 1 ns while it lives (PR_SET_TIMERSLACK is per
// thread; the caller's value is restored).
struct FineSleep {
    long prev = -1;
    FineSleep() {
        prev = prctl(PR_GET_TIMERSLACK, 0, 0, 0, 0);
        if (prev > 1) (void)prctl(PR_SET_TIMERSLACK, 1UL, 0, 0, 0);
    }
    ~FineSleep() {
        if (prev > 1) (void)prctl(PR_SET_TIMERSLACK, (unsigned long)prev, 0, 0, 0);
    }
};

// How long tagged result words may trail their stream's completion (µs).
constexpr int64_t kLandGraceUs = 2000;

// Poll scan() (pause between reads) for up to `us` microseconds.
template <typename S>
bool scan_until(S& scan, int64_t us) {
    const auto t0 = std::chrono::steady_clock::now();
    while (!scan()) {
        if (std::chrono::steady_clock::now() - t0 > std::chrono::microseconds(us)) return false;
        for (int k = 0; k < 8; ++k) cpu_relax();
    }
    return true;
}

// Wait until the `per` tagged words of each of `n` workgroups (slots w[per
// b + h]) carry `tag`; x[h] = XOR of their low words. `bytes`: the call's
// payload (the sleep-ahead estimate). kernel + what: the error text.
int wait_tagged(RoutedStream* r, uint32_t tag, uint32_t n, uint32_t* x, uint32_t per, uint64_t bytes,
                const char* kernel, const char* what) {
    using clk = std::chrono::steady_clock;
    const volatile uint64_t* w = static_cast<const volatile uint64_t*>(r->h);
    const uint32_t total = n * per;
    uint32_t done = 0;
    auto scan = [&] {
        while (done < total && (uint32_t)(w[done] >> 32) == tag) {
            x[done % per] ^= (uint32_t)w[done];
            ++done;
        }
        return done == total;
    };
    const uint32_t pol = g_routed_wait.load(std::memory_order_relaxed);
    const uint32_t spin_us = pol & 0xffffu;
    const double expect_us = (double)bytes / kNominalBytesPerUs;
    if (scan()) return 0;
    std::unique_ptr<FineSleep> fine;
    if ((pol >> 16) && expect_us > (double)spin_us + 20.0) {
        fine.reset(new FineSleep);
        std::this_thread::sleep_for(std::chrono::microseconds((int64_t)(0.85 * expect_us)));
    }
    const auto t0 = clk::now();
    while (!scan()) {
        if (clk::now() - t0 > std::chrono::microseconds(spin_us)) break;
        for (int k = 0; k < 8; ++k) cpu_relax();
    }
    if (done == total) return 0;
    if (!fine) fine.reset(new FineSleep);
    for (uint32_t slice = 1;; ++slice) {
        std::this_thread::sleep_for(std::chrono::microseconds(10));
        if (scan()) return 0;
        if (slice % 10 == 0) {
            const hipError_t q = hipStreamQuery(r->st);
            if (q == hipErrorNotReady) continue;
            // finished (or failed) without every tag seen yet. The stream's
            // completion can reach the host BEFORE the kernel's last
            // system-scope stores (the command processor's signal and the
            // shader's writes take different paths over the host link;
            // scripts/soak_service.py saw it 4 times in 1.2 M calls under
            // load), so the words get a grace period before the verdict.
            const hipError_t e = hipStreamSynchronize(r->st);
            if (e == hipSuccess && q == hipSuccess && scan_until(scan, kLandGraceUs)) return 0;
            return hip_fail(e != hipSuccess ? e : (q != hipSuccess ? q : hipErrorUnknown), kernel, what);
        }
    }
}

// A small buffer on a routed stream: W::kWords tagged words per workgroup,
// assembled by W::routed_result.
template <typename W>
int routed_small(int dev, const typename W::Small& sa0, uint32_t sgrid, typename W::T* crc_out) {
    RoutedStream* r = nullptr;
    if (int rc = routed_lease(dev, &r)) return rc;
    typename W::Small sa = sa0;
    int rc = small_image<W>(dev, &sa.image);
    if (!rc) {
        r->tag = r->tag == 0xffffffffu ? 1u : r->tag + 1u;
        sa.tag = r->tag;
        // the previous call on this stream saw all its slots land: nothing
        // writes them now, and no slot can carry this tag before the launch
        memset(r->h, 0, 8ull * W::kWords * sgrid);
        sa.slots = static_cast<decltype(sa.slots)>(r->d);
        hipLaunchKernelGGL((W::template small_kernel<kSmallLanes, kSmallRows>()), dim3(sgrid), dim3(256), 0, r->st,
                           sa);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) rc = hip_fail(e, W::kKernel, "_small_kernel launch");
    }
    if (!rc) {
        uint32_t x[2] = {0, 0};
        rc = wait_tagged(r, sa.tag, sgrid, x, W::kWords, sa.eoff, W::kKernel, "_small_kernel (routed)");
        if (!rc) *crc_out = W::routed_result(x, /*raw=*/true);
    } else {
        (void)hipStreamSynchronize(r->st);  // nothing left running on a returned stream
    }
    routed_return(r);
    return rc;
}

// A long buffer on a routed stream: the last workgroup's tagged result words
// (long_reduce) are spun on like the small kernels' words.
template <typename W>
int routed_long(int dev, const uint8_t* p, uint64_t n, typename W::T crc, typename W::T* crc_out) {
    RoutedStream* r = nullptr;
    if (int rc = routed_lease(dev, &r)) return rc;
    int cus = 0;
    int rc = current_device(&cus) < 0 ? -ENODEV : 0;
    uint32_t tag = 0;
    if (!rc) {
        r->tag = r->tag == 0xffffffffu ? 1u : r->tag + 1u;
        tag = r->tag;
        memset(r->h, 0, 8 * W::kWords);
        rc = extend_device_big<W>(dev, p, n, crc, static_cast<typename W::T*>(r->d), r->st, cus, tag);
    }
    if (!rc) {
        uint32_t x[2] = {0, 0};
        rc = wait_tagged(r, tag, 1, x, W::kWords, n, W::kKernel, " mid/long kernel (routed)");
        if (!rc) {
            *crc_out = W::routed_result(x, /*raw=*/false);
        } else {
            char buf[128];
            W::routed_diag(buf, sizeof buf, static_cast<const volatile uint64_t*>(r->h), tag);
            g_err += buf + long_state_diag(r->st);
        }
    } else {
        (void)hipStreamSynchronize(r->st);
    }
    routed_return(r);
    return rc;
}

// The resident small-buffer services (crc32c_kernels.h
// crc32c_small_service_kernel, crc64_kernels.h crc64_small_service_kernel;
// on by default, photon_crc_set_small_service). One per device and CRC width, each
// started by the first routed call of its width: a non-blocking stream, the
// doorbell, the pinned slot area, the last seq posted. One call at a time
// uses a service (try-lock: a call that finds it busy, or not running, takes
// the launch path, routed_small); the first call after it
// ended starts a new launch and is its first request.
struct SmallService {
    std::mutex mu;
    int kind = 0;              // 0 CRC32C, 1 CRC-64/ECMA
    hipStream_t st = nullptr;
    uint64_t* h = nullptr;     // host view of the pinned area (quit, slots)
    uint64_t* d = nullptr;     // its device view
    uint64_t* vram = nullptr;  // uncached device memory the host writes through the BAR at the same
                               // address (large BAR, mapping verified by bar_host_rw), else null
    // the doorbell of the current launch: vram, or the pinned area (h / d);
    // chosen at each launch, read without the lock by svc_yield
    std::atomic<uint64_t*> bell{nullptr};
    uint64_t* bell_d = nullptr;
    uint32_t seq = 0;          // last seq posted (never 0)
    std::atomic<bool> live{false};  // a launch that has not been seen to end
};
std::atomic<int> g_svc_live{0};  // services with live == true (svc_yield's fast path)
void set_live(SmallService* s, bool on) {
    if (s->live.exchange(on) != on) g_svc_live.fetch_add(on ? 1 : -1, std::memory_order_relaxed);
}

// Doorbell words from the host; the BAR mapping is write-combined: the
// stores leave the CPU at the sfence.
inline void bell_put(SmallService* s, uint32_t i, uint64_t v) {
    __atomic_store_n(s->bell.load(std::memory_order_relaxed) + i, v, __ATOMIC_RELAXED);
}
inline void bell_flush() { __builtin_ia32_sfence(); }
PerDevice<SmallService*> g_svc[2];
std::mutex g_svc_list_mu;
std::vector<SmallService*> g_svc_list;

// Does the host reach device memory p (8 bytes) at the same address, for
// reads and writes? hipDeviceAttributeIsLargeBar does not prove it (a VF or a
// container may leave the VRAM unmapped for the CPU), and a plain access to an
// unmapped address would fault inside a drop-in call that has no error
// channel. The kernel's copy to and from a pipe touches p instead: an
// unmapped p gives EFAULT, never a signal. A device-side write is
// read back by the host, a host write by the device.
bool bar_host_rw(uint64_t* p, hipStream_t st) {
    int fd[2];
    if (pipe2(fd, O_CLOEXEC) != 0) return false;
    bool ok = false;
    do {
        uint64_t got = 0, back = 0;
        const uint64_t dev_word = 0xA5A5A5A5A5A5A5A5ull, host_word = 0x5AC3C3A55AC3C3A5ull;
        if (hipMemsetAsync(p, 0xA5, 8, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess) break;
        if (write(fd[1], p, 8) != 8 || read(fd[0], &got, 8) != 8 || got != dev_word) break;
        if (write(fd[1], &host_word, 8) != 8 || read(fd[0], p, 8) != 8) break;
        bell_flush();
        if (hipMemcpyAsync(&back, p, 8, hipMemcpyDeviceToHost, st) != hipSuccess ||
            hipStreamSynchronize(st) != hipSuccess || back != host_word)
            break;
        ok = true;
    } while (false);
    close(fd[0]);
    close(fd[1]);
    return ok;
}

// Tell a live service to end and wait for its waves (caller holds s->mu).
void service_end(SmallService* s) {
    if (!s->live) return;
    bell_put(s, kSvcStop, 1ull);
    bell_flush();
    (void)hipStreamSynchronize(s->st);
    set_live(s, false);
}

void service_end_all() {
    std::lock_guard<std::mutex> lk(g_svc_list_mu);
    for (SmallService* s : g_svc_list) {
        std::lock_guard<std::mutex> l2(s->mu);
        int prev = -1;
        (void)hipGetDevice(&prev);
        int dev = -1;
        if (hipStreamGetDevice(s->st, &dev) == hipSuccess) (void)hipSetDevice(dev);
        service_end(s);
        if (prev >= 0) (void)hipSetDevice(prev);
    }
}

// At process exit (atexit): stop every running launch and wait, bounded, for
// each workgroup's exit word -- no HIP call, since a profiler's or the
// runtime's own exit hooks may already have run (rocprofv3 aborted in one:
// "get_stream_stack() must be non nullptr" inside hipStreamSynchronize).
void service_end_at_exit() {
    std::lock_guard<std::mutex> lk(g_svc_list_mu);
    for (SmallService* s : g_svc_list) {
        std::lock_guard<std::mutex> l2(s->mu);
        if (!s->live) continue;
        volatile uint64_t* h = s->h;
        if (!h[kSvcQuit]) {
            bell_put(s, kSvcStop, 1ull);
            bell_flush();
        }
        const auto t0 = std::chrono::steady_clock::now();
        for (uint32_t b = 0; b < kSmallWg;) {
            if (h[kSvcSlots + kSvcSlotStride * b + kSvcExitWord]) {
                ++b;
                continue;
            }
            if (std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(50)) break;
            cpu_relax();
        }
        set_live(s, false);
    }
}

int service_get(int dev, int kind, SmallService** out) {
    return g_svc[kind].get(dev, out, [kind](int, SmallService*& slot) {
        auto* s = new SmallService;
        s->kind = kind;
        const uint64_t bytes = 8 * kSvcWords + (PCRC_SVC_STAMP ? 128 * kSmallWg : 0);
        const hipError_t e = relaxed_capture([&] {
            // A hardware queue of its own: HIP multiplexes streams of one
            // priority onto GPU_MAX_HW_QUEUES (4) queues, and a stream that
            // shared the service's queue would wait behind the resident launch
            // until its idle time ends (seen: a routed launch took the service's
            // 20 ms idle time once enough streams existed). The greatest
            // priority has a queue pool of its own (non-blocking, like the rest).
            int least = 0, greatest = 0;
            hipError_t r = hipDeviceGetStreamPriorityRange(&least, &greatest);
            if (r == hipSuccess) r = hipStreamCreateWithPriority(&s->st, hipStreamNonBlocking, greatest);
            if (r == hipSuccess)
                r = hipHostMalloc(reinterpret_cast<void**>(&s->h), bytes,
                                  hipHostMallocMapped | hipHostMallocPortable | hipHostMallocCoherent);
            if (r == hipSuccess) r = hipHostGetDevicePointer(reinterpret_cast<void**>(&s->d), s->h, 0);
            int dev = 0, large_bar = 0;
            if (r == hipSuccess) r = hipGetDevice(&dev);
            if (r == hipSuccess && hipDeviceGetAttribute(&large_bar, hipDeviceAttributeIsLargeBar, dev) == hipSuccess &&
                large_bar == 1 &&
                hipExtMallocWithFlags(reinterpret_cast<void**>(&s->vram), 4096, hipDeviceMallocUncached) == hipSuccess) {
                if (!bar_host_rw(s->vram, s->st)) {  // not mapped for the host here: the pinned doorbell
                    (void)hipFree(s->vram);
                    s->vram = nullptr;
                }
                if (s->vram) r = hipMemsetAsync(s->vram, 0, 4096, s->st);  // complete before the host writes it
                if (r == hipSuccess) r = hipStreamSynchronize(s->st);
            }
            (void)hipGetLastError();
            return r;
        });
        if (e != hipSuccess) {
            if (s->vram) (void)hipFree(s->vram);
            if (s->h) (void)hipHostFree(s->h);
            if (s->st) (void)hipStreamDestroy(s->st);
            delete s;
            return hip_fail(e, "small-buffer service");
        }
        memset(s->h, 0, bytes);
        s->bell.store(s->h, std::memory_order_relaxed);  // until the first launch picks its doorbell
        s->bell_d = s->d;
        std::lock_guard<std::mutex> lk(g_svc_list_mu);
        if (g_svc_list.empty()) atexit(service_end_at_exit);  // after HIP's init: runs before its teardown
        g_svc_list.push_back(s);
        g_svc_made.fetch_add(1, std::memory_order_relaxed);
        slot = s;
        return 0;
    });
}

int service_doorbell_of(int dev, int kind) {
    SmallService* s = g_svc[kind].peek(dev);
    if (!s) return -ENOENT;
    return s->bell.load(std::memory_order_relaxed) == s->h ? 0 : 1;
}

void services_end_on_impl(int dev) {
    if (g_svc_live.load(std::memory_order_relaxed) == 0) return;
    for (int kind = 0; kind < 2; ++kind) {
        SmallService* s = g_svc[kind].peek(dev);
        if (!s || !s->live.load()) continue;
        std::lock_guard<std::mutex> lk(s->mu);  // a call in flight finishes first
        service_end(s);
    }
}

// Every batch / message / long launch ends the services first (HeavyLaunch;
// VERDICT r5 #2): deciding co-residency by LDS alone ignored VGPRs
// and wave slots. A routed call starts a new service once the launch has
// finished (heavy_in_flight); until then it takes the launch path.
void svc_yield() {
    if (g_svc_live.load(std::memory_order_relaxed) == 0) return;
    int dev = -1;
    if (hipGetDevice(&dev) != hipSuccess) return;
    for (int kind = 0; kind < 2; ++kind) {
        SmallService* s = g_svc[kind].peek(dev);
        if (!s || !s->live.load()) continue;
        // no lock: a call in flight sees quit, waits for the stream and takes
        // the launch path; the next call starts a new launch
        bell_put(s, kSvcStop, 1ull);
        bell_flush();
        __atomic_store_n(&s->h[kSvcQuit], 1ull, __ATOMIC_RELAXED);
    }
}

// The ring of a device's last kHeavyEvents heavy launches (HeavyLaunch),
// kept only while device dispatch is on or once a service exists (a process
// without routed calls pays nothing). Launches captured into a graph are not
// marked, and a launch older than the last kHeavyEvents may still run
// unmarked (many streams at once); a service started beside such a launch
// only costs it CUs, for at most the service's life -- never a wrong CRC.
constexpr int kHeavyEvents = 8;
struct HeavyRing {
    std::mutex mu;
    hipEvent_t ev[kHeavyEvents] = {};
    bool pending[kHeavyEvents] = {};
    uint32_t next = 0;
};
PerDevice<HeavyRing*> g_heavy;

void heavy_mark(hipStream_t st) {
    if (!g_dispatch_on.load(std::memory_order_relaxed) && g_svc_made.load(std::memory_order_relaxed) == 0) return;
    int dev = -1;
    if (hipGetDevice(&dev) != hipSuccess) return;
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(st, &cs) != hipSuccess || cs != hipStreamCaptureStatusNone) {
        (void)hipGetLastError();  // never left for the caller's next launch check
        return;
    }
    HeavyRing* r = nullptr;
    if (g_heavy.get(dev, &r, [](int, HeavyRing*& slot) {
            auto* h = new HeavyRing;
            const hipError_t e = relaxed_capture([&] {
                hipError_t x = hipSuccess;
                for (int i = 0; i < kHeavyEvents && x == hipSuccess; ++i)
                    x = hipEventCreateWithFlags(&h->ev[i], hipEventDisableTiming);
                return x;
            });
            if (e != hipSuccess) {
                for (hipEvent_t ev : h->ev)
                    if (ev) (void)hipEventDestroy(ev);
                delete h;
                (void)hipGetLastError();
                return -EIO;
            }
            slot = h;
            return 0;
        }))
        return;
    std::lock_guard<std::mutex> lk(r->mu);
    const uint32_t i = r->next++ % kHeavyEvents;
    r->pending[i] = hipEventRecord(r->ev[i], st) == hipSuccess;
    if (!r->pending[i]) (void)hipGetLastError();
}

// Is a heavy launch marked on `dev` still queued or running?
bool heavy_in_flight(int dev) {
    HeavyRing* r = g_heavy.peek(dev);
    if (!r) return false;
    std::lock_guard<std::mutex> lk(r->mu);
    bool busy = false;
    for (int i = 0; i < kHeavyEvents; ++i) {
        if (!r->pending[i]) continue;
        if (hipEventQuery(r->ev[i]) == hipErrorNotReady)
            busy = true;
        else
            r->pending[i] = false;
    }
    return busy;
}

// Serve one routed small call through the service of its width: 0 = the
// slots' XOR is in x[0] (CRC-64: x[1] the high words), 1 = not served (take
// the launch path). The request: a0, nb, s0, k, wg0, eoff as small_args
// computed them, seed (W::seed_word; CRC-64: the inverted init).
int service_small(int dev, int kind, const uint8_t* a0, uint32_t nb, uint32_t s0, uint32_t k, uint32_t wg0,
                  uint32_t eoff, uint64_t seed, uint32_t x[2]) {
    const int idle_us = g_svc_idle_us.load(std::memory_order_relaxed);
    if (idle_us <= 0 || g_fail_next > 0) return 1;  // an injected failure (tuning.h) hits the launch path
    SmallService* s = nullptr;
    if (service_get(dev, kind, &s)) return 1;
    std::unique_lock<std::mutex> lk(s->mu, std::try_to_lock);
    if (!lk.owns_lock()) return 1;
    volatile uint64_t* h = s->h;
    if (s->live && h[kSvcQuit]) {  // it ended (idle / life / svc_yield): its waves leave at their next poll
        (void)hipStreamSynchronize(s->st);
        set_live(s, false);
    }
    if (!s->live) {
        if (heavy_in_flight(dev)) {  // a batch / long launch holds the CUs: the launch path
            g_svc_deferred.fetch_add(1, std::memory_order_relaxed);
            return 1;
        }
        const void* img = nullptr;
        if (kind == 0) {
            const uint32_t* i32 = nullptr;
            if (small_image<Crc32c>(dev, &i32)) return 1;
            img = i32;
        } else {
            const uint64_t* i64 = nullptr;
            if (small_image<Crc64>(dev, &i64)) return 1;
            img = i64;
        }
        // this launch's doorbell; its request words carry the last seq posted
        // (never taken as fresh), whichever doorbell the last launch used
        const bool bar = s->vram && g_svc_bell.load(std::memory_order_relaxed);
        s->bell.store(bar ? s->vram : s->h, std::memory_order_relaxed);
        s->bell_d = bar ? s->vram : s->d;
        for (uint32_t i = 0; i < kSvcStop; ++i) bell_put(s, i, (uint64_t)s->seq << 32);
        bell_put(s, kSvcStop, 0ull);
        bell_put(s, kSvcQuit, 0ull);
        bell_flush();
        __atomic_store_n(&s->h[kSvcQuit], 0ull, __ATOMIC_RELAXED);
        for (uint32_t b = 0; b < kSmallWg; ++b)  // the last launch's waves have all left (stream synchronised)
            __atomic_store_n(&s->h[kSvcSlots + kSvcSlotStride * b + kSvcExitWord], 0ull, __ATOMIC_RELAXED);
        const uint32_t life = 100u * (uint32_t)g_svc_life_us.load(std::memory_order_relaxed);
        ServiceArgs a{img, s->bell_d, s->d, s->seq, 100u * (uint32_t)idle_us, life};
        const hipError_t e = relaxed_capture([&] {
            if (kind == 0)
                hipLaunchKernelGGL(crc32c_small_service_kernel, dim3(kSmallWg), dim3(256), 0, s->st, a);
            else
                hipLaunchKernelGGL(crc64_small_service_kernel, dim3(kSmallWg), dim3(256), 0, s->st, a);
            return hipGetLastError();
        });
        if (e != hipSuccess) return 1;
        set_live(s, true);
        g_svc_starts.fetch_add(1, std::memory_order_relaxed);
        // and this call is the new launch's first request: it pays the launch
        // either way, and a call over 256 KiB sent to the launch path instead
        // would take the long kernel, whose svc_yield ends the launch again
    }
    uint32_t seq = s->seq + 1u;
    if (seq == 0) seq = 1;
    s->seq = seq;
    const uint64_t tag = (uint64_t)seq << 32;
    const uint64_t f[kSvcStop] = {(uint32_t)reinterpret_cast<uintptr_t>(a0),
                                  (uint32_t)(reinterpret_cast<uintptr_t>(a0) >> 32),
                                  nb | s0 << 20 | k << 24,
                                  eoff | wg0 << 26,
                                  (uint32_t)seed,
                                  (uint32_t)(seed >> 32)};
    for (uint32_t i = 0; i < kSvcStop; ++i) bell_put(s, i, tag | f[i]);
    bell_flush();
    const uint32_t per = kind ? 2 : 1, n = per * (kSmallWg - wg0);
    uint32_t done = 0;
    x[0] = x[1] = 0;
    auto scan = [&] {
        while (done < n) {
            const uint64_t v = h[kSvcSlots + kSvcSlotStride * (wg0 + done / per) + done % per];
            if ((v >> 32) != seq) break;
            x[done % per] ^= (uint32_t)v;
            ++done;
        }
        return done == n;
    };
    // as wait_tagged: a pause-polled window, then 10 µs sleeps; a service seen
    // to end (quit set, or its stream done) without every slot: not served
    using clk = std::chrono::steady_clock;
    const auto t0 = clk::now();
    const uint32_t spin_us = g_routed_wait.load(std::memory_order_relaxed) & 0xffffu;
    std::unique_ptr<FineSleep> fine;
    while (!scan()) {
        if (clk::now() - t0 < std::chrono::microseconds(spin_us)) {
            for (int j = 0; j < 8; ++j) cpu_relax();
            continue;
        }
        if (!fine) fine.reset(new FineSleep);
        std::this_thread::sleep_for(std::chrono::microseconds(10));
        if (h[kSvcQuit] || hipStreamQuery(s->st) != hipErrorNotReady) {
            (void)hipStreamSynchronize(s->st);  // every wave has left: the slots are final once they land
            set_live(s, false);
            if (scan_until(scan, kLandGraceUs / 10)) break;
            g_svc_missed.fetch_add(1, std::memory_order_relaxed);
            return 1;
        }
    }
    g_svc_served.fetch_add(1, std::memory_order_relaxed);
    return 0;
}

// The routed crc32c_extend / crc64ecma_extend.
template <typename W>
typename W::T dispatch_crc(const uint8_t* p, size_t n, typename W::T crc) {
    const int dev = n ? device_of(p) : -1;
    if (dev < 0) return host_engine(&W::host_crc)(p, n, crc);
    DeviceScope scope(dev);
    typename W::T r = 0;
    typename W::Small sa{};
    uint32_t sgrid = 0;
    int rc;
    uint32_t x[2];
    if (small_args<W>(p, n, crc, &sa, &sgrid, kSvcMaxBlocks) &&
        service_small(dev, W::kService, sa.a0, sa.nb, sa.s0, sa.k, sa.wg0, sa.eoff, W::seed_word(sa), x) == 0) {
        r = W::routed_result(x, /*raw=*/true);  // per-workgroup words in pinned memory, XORed by service_small
        rc = 0;
    } else if (sa.nb && sa.nb <= kSmallBlocks) {
        rc = routed_small<W>(dev, sa, sgrid, &r);
    } else {
        rc = routed_long<W>(dev, p, n, crc, &r);
    }
    if (!rc) return r;
    routed_failure(W::kExtend, rc);
    return host_crc_of_device<W>(p, n, crc);
}

// The routed crc32c_series / crc64ecma_series: run(out, stream) enqueues the
// device form.
template <typename W, typename R>
void dispatch_series_with(const uint8_t* buf, uint32_t part, uint32_t n, typename W::T* parts, R run) {
    typedef typename W::T T;
    const int dev = (part && n) ? device_of(buf) : -1;
    if (dev < 0) return host_engine(&W::host_series)(buf, part, n, parts);
    DeviceScope scope(dev);
    const bool parts_on_dev = device_of(parts) == dev;
    int rc;
    if (parts_on_dev) {
        RoutedStream* r = nullptr;
        rc = routed_lease(dev, &r);
        if (!rc) {
            rc = run(parts, r->st);
            hipError_t e = hipStreamSynchronize(r->st);
            if (!rc && e != hipSuccess) rc = hip_fail(e, "hipStreamSynchronize");
            routed_return(r);
        }
    } else {
        rc = with_scratch(dev, sizeof(T) * n, parts, sizeof(T) * n,
                          [&](void* d, hipStream_t st) { return run(static_cast<T*>(d), st); });
    }
    if (!rc) return;
    routed_failure(W::kSeries, rc);
    std::vector<T> h(n);
    uint64_t i = 0;
    std::vector<uint8_t> part_buf;
    for_host_chunks(buf, (size_t)part * n, W::kSeries, [&](const uint8_t* hp, size_t k) {
        // whole parts only: gather across chunk edges into part_buf
        part_buf.insert(part_buf.end(), hp, hp + k);
        size_t whole = part_buf.size() / part;
        host_engine(&W::host_series)(part_buf.data(), part, (uint32_t)whole, h.data() + i);
        i += whole;
        part_buf.erase(part_buf.begin(), part_buf.begin() + whole * part);
    });
    if (parts_on_dev) {
        hipError_t e = hipMemcpy(parts, h.data(), sizeof(T) * n, hipMemcpyHostToDevice);
        if (e != hipSuccess) routed_abort(W::kSeries, e);
    } else {
        memcpy(parts, h.data(), sizeof(T) * n);
    }
}

void dispatch_series(const uint8_t* buf, uint32_t part, uint32_t n, uint32_t* parts) {
    // The device form keeps the SSE4.2 engine's rule (parts < 8 B give 0,
    // crc.cpp:481-500); when the saved host engine is crc32c_series_sw those
    // parts get their real CRCs (crc.cpp:474-478), so run the plain batch.
    dispatch_series_with<Crc32c>(buf, part, n, parts, [&](uint32_t* out, hipStream_t st) {
        return host_engine(&Crc32c::host_series) == crc32c_series_sw
                   ? photon_crc32c_batch_strided(buf, part, part, n, 0, nullptr, out, st)
                   : photon_crc32c_series_device(buf, part, n, out, st);
    });
}

// The host engines have no part_size quirk (crc64_cpu.cpp), so there is no
// engine to select.
void dispatch_series64(const uint8_t* buf, uint32_t part, uint32_t n, uint64_t* parts) {
    dispatch_series_with<Crc64>(buf, part, n, parts, [&](uint64_t* out, hipStream_t st) {
        return photon_crc64ecma_series_device(buf, part, n, out, st);
    });
}

// The routed crc32c_combine_series / crc64ecma_combine_series.
template <typename W>
typename W::T dispatch_combine_series(typename W::T* crc, uint32_t part, uint32_t n) {
    typedef typename W::T T;
    const int dev = n ? device_of(crc) : -1;
    if (dev < 0) return host_engine(&W::host_cseries)(crc, part, n);
    DeviceScope scope(dev);
    T r = 0;  // device scratch, not the pinned word: the kernel accumulates with device atomics
    int rc = with_scratch(dev, sizeof(T), &r, sizeof(T), [&](void* d, hipStream_t st) {
        return combine_series_device<W>(crc, part, n, static_cast<T*>(d), st);
    });
    if (!rc) return r;
    routed_failure(W::kCombineSeries, rc);
    std::vector<T> h(n);
    hipError_t e = hipMemcpy(h.data(), crc, sizeof(T) * n, hipMemcpyDeviceToHost);
    if (e != hipSuccess) routed_abort(W::kCombineSeries, e);
    return host_engine(&W::host_cseries)(h.data(), part, n);
}


}  // namespace
}  // namespace pcrc

// The reference writes its dispatch pointers once, before main (crc.cpp:137-175),
// and callers read them with plain loads through the inline wrappers of
// crc32c.h (which this library keeps unchanged). Switching them at run time
// while other threads call through them is therefore done
// with single aligned RELEASE stores of whole pointers: a concurrent caller
// loads either the old or the new engine -- never a torn pointer -- and both
// give the same CRC for every input (the routed wrappers send host pointers
// to the saved host engine, which is published before the routed pointer and
// never cleared). A caller that loaded the routed pointer just before a
// switch-off still runs the routed wrapper once, with the same result.
extern "C" int photon_crc_set_device_dispatch(int on) {
    using namespace pcrc;
    std::lock_guard<std::mutex> lk(g_dispatch_mu);
    if (on && !g_dispatch_on) {
        __atomic_store_n(&Crc32c::host_crc, __atomic_load_n(&crc32c_auto, __ATOMIC_ACQUIRE), __ATOMIC_RELAXED);
        __atomic_store_n(&Crc32c::host_series, __atomic_load_n(&crc32c_series_auto, __ATOMIC_ACQUIRE),
                         __ATOMIC_RELAXED);
        __atomic_store_n(&Crc32c::host_cseries, __atomic_load_n(&crc32c_combine_series_auto, __ATOMIC_ACQUIRE),
                         __ATOMIC_RELAXED);
        __atomic_store_n(&Crc64::host_crc, __atomic_load_n(&crc64ecma_auto, __ATOMIC_ACQUIRE), __ATOMIC_RELAXED);
        __atomic_store_n(&Crc64::host_series, __atomic_load_n(&crc64ecma_series_auto, __ATOMIC_ACQUIRE),
                         __ATOMIC_RELAXED);
        __atomic_store_n(&Crc64::host_cseries, __atomic_load_n(&crc64ecma_combine_series_auto, __ATOMIC_ACQUIRE),
                         __ATOMIC_RELAXED);
        __atomic_store_n(&crc32c_auto, &dispatch_crc<Crc32c>, __ATOMIC_RELEASE);
        __atomic_store_n(&crc32c_series_auto, &dispatch_series, __ATOMIC_RELEASE);
        __atomic_store_n(&crc32c_combine_series_auto, &dispatch_combine_series<Crc32c>, __ATOMIC_RELEASE);
        __atomic_store_n(&crc64ecma_auto, &dispatch_crc<Crc64>, __ATOMIC_RELEASE);
        __atomic_store_n(&crc64ecma_series_auto, &dispatch_series64, __ATOMIC_RELEASE);
        __atomic_store_n(&crc64ecma_combine_series_auto, &dispatch_combine_series<Crc64>, __ATOMIC_RELEASE);
        g_dispatch_on = true;
    } else if (!on && g_dispatch_on) {
        __atomic_store_n(&crc32c_auto, Crc32c::host_crc, __ATOMIC_RELEASE);
        __atomic_store_n(&crc32c_series_auto, Crc32c::host_series, __ATOMIC_RELEASE);
        __atomic_store_n(&crc32c_combine_series_auto, Crc32c::host_cseries, __ATOMIC_RELEASE);
        __atomic_store_n(&crc64ecma_auto, Crc64::host_crc, __ATOMIC_RELEASE);
        __atomic_store_n(&crc64ecma_series_auto, Crc64::host_series, __ATOMIC_RELEASE);
        __atomic_store_n(&crc64ecma_combine_series_auto, Crc64::host_cseries, __ATOMIC_RELEASE);
        g_dispatch_on = false;
    }
    return g_dispatch_err.exchange(0) ? -EIO : 0;
}

extern "C" uint64_t photon_crc_dispatch_fallbacks(void) { return pcrc::g_fallbacks.load(); }

#if PCRC_SVC_STAMP
// bench-only builds: the current device's service area (host view)
extern "C" void* photon_crc_test_service_area(void) {
    int dev = 0;
    (void)hipGetDevice(&dev);
    pcrc::SmallService* s = nullptr;
    return pcrc::service_get(dev, 0, &s) ? nullptr : s->h;
}
#endif

// internal.h: for the vDMA initiator's device-wide fence (vdma_hip.cpp).
void pcrc::services_end_on(int dev) { services_end_on_impl(dev); }
void pcrc::services_end_before_free() {
    if (pcrc::g_svc_live.load(std::memory_order_relaxed)) pcrc::service_end_all();
}
