// file_source.cpp -- the runtime shim (streams, device memory, copies,
// completion callbacks: Photon code needs no HIP headers) and producers of
// checksum input outside device memory
// (include/photon_crc/crc32c_gpu.h):
//   photon_crc_host_register / _unregister: make existing host buffers (e.g.
//       the iovec targets of IFile::preadv, fs/filesystem.h:54-70) readable by
//       the kernels in place (hipHostRegister, mapped);
//   photon_crc32c_file_strided: checksum equal-size records of a file. A
//       reader thread pread()s 4 KiB-aligned chunks (O_DIRECT-compatible) into
//       two pinned chunk buffers while the GPU pipeline
//       (photon_crc32c_host_batch_strided) checksums the previous chunk, so
//       the CPU never touches the payload bytes when the fd is O_DIRECT.
#include <errno.h>
#include <hip/hip_runtime_api.h>
#include <stdint.h>
#include <string.h>
#include <unistd.h>

#include <atomic>
#include <vector>
#include <map>
#include <mutex>
#include <string>

#include <photon_crc/crc32c_gpu.h>
#include <photon_crc/tuning.h>

#include "host_chunks.h"
#include "internal.h"

namespace {

using pcrc::report_error;
using pcrc::report_hip_error;

constexpr int kKeepPairs = 4;  // chunk-buffer pairs kept pinned between calls

// Payload span per chunk of photon_crc32c_file_strided, 0 = the default
// (host_chunks.h kFileChunk; photon_crc_set_file_chunk_bytes, tests).
std::atomic<uint64_t> g_file_chunk{0};

// A pair of pinned chunk buffers, owned by ONE call at a time: concurrent
// callers check out their own pair (pinned allocation is slow, so pairs are
// kept for reuse), so they no longer serialise on one global pair.
struct ChunkPair {
    void* buf[2] = {nullptr, nullptr};
    uint64_t cap = 0;
};

struct PairCache {
    std::mutex mu;
    std::vector<ChunkPair> free;
};

PairCache& pair_cache() {
    static PairCache* c = new PairCache;
    return *c;
}

void free_pair(ChunkPair& p) {
    for (void*& b : p.buf)
        if (b) {
            (void)hipHostFree(b);
            b = nullptr;
        }
    p.cap = 0;
}

int checkout_pair(uint64_t cap, ChunkPair* out) {
    {
        PairCache& c = pair_cache();
        std::lock_guard<std::mutex> lk(c.mu);
        for (size_t i = 0; i < c.free.size(); ++i)
            if (c.free[i].cap >= cap) {
                *out = c.free[i];
                c.free.erase(c.free.begin() + i);
                return 0;
            }
    }
    ChunkPair p;
    for (void*& b : p.buf) {
        hipError_t e = hipHostMalloc(&b, cap, hipHostMallocPortable);
        if (e != hipSuccess) {
            free_pair(p);
            return report_hip_error(e, "hipHostMalloc(chunk)");
        }
    }
    p.cap = cap;
    *out = p;
    return 0;
}

void return_pair(ChunkPair p) {
    PairCache& c = pair_cache();
    std::lock_guard<std::mutex> lk(c.mu);
    c.free.push_back(p);
    if ((int)c.free.size() > kKeepPairs) {  // drop the smallest
        size_t k = 0;
        for (size_t i = 1; i < c.free.size(); ++i)
            if (c.free[i].cap < c.free[k].cap) k = i;
        free_pair(c.free[k]);
        c.free.erase(c.free.begin() + k);
    }
}

// Ranges registered through photon_crc_host_register, so the message batch
// can check that a segment [p, p+n) stays inside its registration (file-local:
// no exported symbol a host application could collide with).
std::mutex g_reg_mu;
std::map<uintptr_t, uint64_t> g_reg;

}  // namespace

void pcrc::record_registration(const void* p, uint64_t n) {
    std::lock_guard<std::mutex> lk(g_reg_mu);
    g_reg[reinterpret_cast<uintptr_t>(p)] = n;
}

void pcrc::forget_registration(const void* p) {
    std::lock_guard<std::mutex> lk(g_reg_mu);
    g_reg.erase(reinterpret_cast<uintptr_t>(p));
}

int pcrc::registered_range_check(const void* p, uint64_t n) {
    const uintptr_t q = reinterpret_cast<uintptr_t>(p);
    std::lock_guard<std::mutex> lk(g_reg_mu);
    auto it = g_reg.upper_bound(q);
    if (it == g_reg.begin()) return -1;
    --it;
    if (q - it->first >= it->second) return -1;  // not inside a known registration
    return n <= it->second - (q - it->first) ? 1 : 0;
}

extern "C" {

int photon_crc_stream_create(void** stream) {
    if (!stream) return report_error(-EINVAL, "null stream pointer");
    if (photon_crc_device_count() <= 0) return -ENODEV;
    hipStream_t s = nullptr;
    hipError_t e = hipStreamCreateWithFlags(&s, hipStreamNonBlocking);
    if (e != hipSuccess) return report_hip_error(e, "hipStreamCreateWithFlags");
    *stream = s;
    return 0;
}

int photon_crc_stream_destroy(void* stream) {
    if (!stream) return 0;
    hipError_t e = hipStreamDestroy(static_cast<hipStream_t>(stream));
    return e == hipSuccess ? 0 : report_hip_error(e, "hipStreamDestroy");
}

int photon_crc_stream_sync(void* stream) {
    if (photon_crc_device_count() <= 0) return -ENODEV;
    hipError_t e = hipStreamSynchronize(static_cast<hipStream_t>(stream));
    return e == hipSuccess ? 0 : report_hip_error(e, "hipStreamSynchronize");
}

int photon_crc_stream_on_complete(void* stream, void (*fn)(void* arg), void* arg) {
    if (!fn) return report_error(-EINVAL, "null callback");
    if (photon_crc_device_count() <= 0) return -ENODEV;
    hipError_t e = hipLaunchHostFunc(static_cast<hipStream_t>(stream), fn, arg);
    return e == hipSuccess ? 0 : report_hip_error(e, "hipLaunchHostFunc");
}

int photon_crc_device_alloc(void** ptr, uint64_t nbytes) {
    if (!ptr || !nbytes) return report_error(-EINVAL, "null pointer or zero size");
    if (photon_crc_device_count() <= 0) return -ENODEV;
    hipError_t e = hipMalloc(ptr, nbytes);
    return e == hipSuccess ? 0 : report_hip_error(e, "hipMalloc");
}

int photon_crc_device_free(void* ptr) {
    if (!ptr) return 0;
    pcrc::services_end_before_free();
    hipError_t e = hipFree(ptr);
    return e == hipSuccess ? 0 : report_hip_error(e, "hipFree");
}

int photon_crc_memcpy_async(void* dst, const void* src, uint64_t nbytes, void* stream) {
    if (!nbytes) return 0;
    if (!dst || !src) return report_error(-EINVAL, "null pointer");
    if (photon_crc_device_count() <= 0) return -ENODEV;
    hipError_t e = hipMemcpyAsync(dst, src, nbytes, hipMemcpyDefault, static_cast<hipStream_t>(stream));
    return e == hipSuccess ? 0 : report_hip_error(e, "hipMemcpyAsync");
}

int photon_crc_host_register(void* ptr, uint64_t len) {
    if (!ptr || !len) return report_error(-EINVAL, "null or empty range");
    hipError_t e = hipHostRegister(ptr, len, hipHostRegisterMapped | hipHostRegisterPortable);
    if (e != hipSuccess) return report_hip_error(e, "hipHostRegister");
    std::lock_guard<std::mutex> lk(g_reg_mu);
    g_reg[reinterpret_cast<uintptr_t>(ptr)] = len;
    return 0;
}

int photon_crc_host_unregister(void* ptr) {
    hipError_t e = hipHostUnregister(ptr);
    if (e != hipSuccess) return report_hip_error(e, "hipHostUnregister");
    std::lock_guard<std::mutex> lk(g_reg_mu);
    g_reg.erase(reinterpret_cast<uintptr_t>(ptr));
    return 0;
}

int photon_crc32c_file_strided(int fd, uint64_t offset, uint64_t stride, uint64_t nbytes, uint64_t count,
                               uint32_t seed0, uint32_t* h_out) {
    if (!count) return 0;
    if (fd < 0 || !h_out || stride < nbytes || !nbytes) return report_error(-EINVAL, "bad arguments");
    if (photon_crc_device_count() <= 0) return -ENODEV;
    // Records per chunk and the chunk buffers' size (host_chunks.h).
    const uint64_t chunk = g_file_chunk.load(std::memory_order_relaxed);
    const pcrc::FilePlan pl = pcrc::file_plan(offset, stride, nbytes, count, chunk ? chunk : pcrc::kFileChunk);
    ChunkPair cb;
    if (int prc = checkout_pair(pl.span_max, &cb)) return prc;
    struct Return {
        ChunkPair& p;
        ~Return() { return_pair(p); }
    } give_back{cb};

    uint8_t* const buf[2] = {static_cast<uint8_t*>(cb.buf[0]), static_cast<uint8_t*>(cb.buf[1])};
    std::string read_err;
    const int rc = pcrc::file_pipeline(
        fd, pl, buf,
        [&](const uint8_t* records, uint64_t first, uint64_t k) {
            return photon_crc32c_host_batch_strided(records, stride, nbytes, k, seed0, nullptr, h_out + first);
        },
        &read_err);
    if (!read_err.empty()) return report_error(rc, read_err.c_str());
    return rc;
}

int photon_crc_set_file_chunk_bytes(uint64_t bytes) {
    if (!pcrc::file_chunk_valid(bytes))
        return report_error(-EINVAL, "file chunk bytes: 0 (default) or a multiple of 4096 up to 64 MiB");
    g_file_chunk.store(bytes, std::memory_order_relaxed);
    return 0;
}

}  // extern "C"
