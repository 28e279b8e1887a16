// host_chunks.h -- the host-side chunking of the two pipelines that feed the
// kernels from outside device memory, free of HIP so that it also runs
// stand-alone on the CPU and under sanitizers
// (tests/cpp/host_chunks_replay.cpp):
//   * the staging plan of the host-memory pipeline (host_batch_impl in
//     crc32c_device.hip: photon_crc32c_host_batch_strided /
//     photon_crc64ecma_host_batch_strided): pitch, buffers per staging chunk,
//     and (first, k, slot) of chunk i;
//   * the chunk geometry of photon_crc32c_file_strided (file_source.cpp):
//     records per chunk, and per chunk the file span read, rounded out to
//     4 KiB (O_DIRECT-compatible), and where record 0 sits in the buffer;
//   * the reads (read_span, the piece cut of read_span_parallel, the
//     persistent ReaderPool) and the two-buffer reader / consumer loop, a
//     template over the consumer so that the library passes its pinned pair
//     and the GPU pipeline, a CPU program malloc'ed buffers and a CPU CRC.
#pragma once
#include <errno.h>
#include <stdint.h>
#include <string.h>
#include <unistd.h>

#include <condition_variable>
#include <deque>
#include <functional>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

namespace pcrc {

// ---------------------------------------------------------------- staging plan
constexpr int kNumStage = 3;
constexpr uint64_t kStageBytes = 256ull << 20;    // a staging allocation, and the default span of a chunk
constexpr uint64_t kStageMinSpan = 64ull << 10;   // photon_crc_set_host_stage_bytes's lower bound

inline bool stage_span_valid(uint64_t bytes) {
    return bytes == 0 || (bytes % 256 == 0 && bytes >= kStageMinSpan && bytes <= kStageBytes);
}

// `count` buffers of nbytes (> 0) packed at `pitch` into staging chunks that
// hold `span` bytes (at most kStageBytes): per_chunk buffers each, one when
// the pitch is above the span (the caller refuses a pitch above the
// allocation, kStageBytes).
struct StagePlan {
    uint64_t pitch;
    uint64_t per_chunk;
    uint64_t nchunks;
    uint64_t count;
};

struct StageChunk {
    uint64_t first;  // index of the chunk's first buffer
    uint64_t k;      // its buffers
    int slot;        // the staging chunk it lands in
};

inline StagePlan stage_plan(uint64_t nbytes, uint64_t count, uint64_t span) {
    StagePlan pl;
    pl.pitch = (nbytes + 255) & ~uint64_t(255);
    pl.per_chunk = span / pl.pitch;
    if (pl.per_chunk == 0) pl.per_chunk = 1;
    pl.nchunks = count / pl.per_chunk + (count % pl.per_chunk != 0);
    pl.count = count;
    return pl;
}

inline StageChunk stage_chunk(const StagePlan& pl, uint64_t i) {
    StageChunk c;
    c.first = i * pl.per_chunk;
    c.k = pl.count - c.first < pl.per_chunk ? pl.count - c.first : pl.per_chunk;
    c.slot = (int)(i % kNumStage);
    return c;
}

// ---------------------------------------------------------------- file geometry
constexpr uint64_t kFileAlign = 4096;
constexpr uint64_t kFileChunk = 64ull << 20;  // payload span per chunk (default, and the upper bound of the knob)
constexpr int kReadPieces = 8;                // parallel preads per chunk (page-cache copies are per-core bound)
constexpr int kReaderThreads = 16;            // persistent reader pool, shared by concurrent callers

inline bool file_chunk_valid(uint64_t bytes) {
    return bytes == 0 || (bytes % kFileAlign == 0 && bytes <= kFileChunk);
}

// `count` (> 0) records of nbytes (> 0) at offset + i * stride (stride >=
// nbytes), `per` records per chunk of `chunk` payload bytes; span_max = the
// bytes a chunk buffer must hold (a chunk's read span is rounded out to 4 KiB).
struct FilePlan {
    uint64_t offset, stride, nbytes, count;
    uint64_t per;
    uint64_t span_max;
    uint64_t nchunks;
};

struct FileChunk {
    uint64_t first, k;  // the chunk's records
    uint64_t lo, hi;    // their bytes in the file
    uint64_t alo, ahi;  // the span read: [lo, hi) rounded out to 4 KiB
    uint64_t skew;      // record `first` sits at buffer + skew
};

inline FilePlan file_plan(uint64_t offset, uint64_t stride, uint64_t nbytes, uint64_t count, uint64_t chunk) {
    FilePlan pl;
    pl.offset = offset;
    pl.stride = stride;
    pl.nbytes = nbytes;
    pl.count = count;
    pl.per = chunk / stride;
    if (pl.per == 0) pl.per = 1;
    if (pl.per > count) pl.per = count;
    pl.span_max = (pl.per - 1) * stride + nbytes + 2 * kFileAlign;
    pl.nchunks = (count + pl.per - 1) / pl.per;
    return pl;
}

inline FileChunk file_chunk(const FilePlan& pl, uint64_t c) {
    FileChunk ch;
    ch.first = c * pl.per;
    ch.k = pl.count - ch.first < pl.per ? pl.count - ch.first : pl.per;
    ch.lo = pl.offset + ch.first * pl.stride;
    ch.hi = ch.lo + (ch.k - 1) * pl.stride + pl.nbytes;
    ch.alo = ch.lo & ~(kFileAlign - 1);
    ch.ahi = (ch.hi + kFileAlign - 1) & ~(kFileAlign - 1);
    ch.skew = ch.lo - ch.alo;
    return ch;
}

// ---------------------------------------------------------------- reads
// Persistent reader threads (created on first use) running pread pieces for
// every caller: no thread start-up per chunk.
class ReaderPool {
public:
    static ReaderPool& get() {
        static ReaderPool* p = new ReaderPool;  // never destroyed: workers outlive static destruction
        return *p;
    }
    // Run every task on the pool and wait for all of them.
    void run_all(std::vector<std::function<void()>>& tasks) {
        std::mutex done_mu;
        std::condition_variable done_cv;
        size_t left = tasks.size();
        {
            std::lock_guard<std::mutex> lk(mu_);
            for (auto& t : tasks)
                q_.push_back([&t, &done_mu, &done_cv, &left] {
                    t();
                    std::lock_guard<std::mutex> g(done_mu);
                    if (--left == 0) done_cv.notify_all();
                });
        }
        cv_.notify_all();
        std::unique_lock<std::mutex> g(done_mu);
        done_cv.wait(g, [&] { return left == 0; });
    }

private:
    ReaderPool() {
        for (int i = 0; i < kReaderThreads; ++i)
            std::thread([this] {
                for (;;) {
                    std::function<void()> job;
                    {
                        std::unique_lock<std::mutex> lk(mu_);
                        cv_.wait(lk, [&] { return !q_.empty(); });
                        job = std::move(q_.front());
                        q_.pop_front();
                    }
                    job();
                }
            }).detach();
    }
    std::mutex mu_;
    std::condition_variable cv_;
    std::deque<std::function<void()>> q_;
};

// Read [off, off+want_max) of fd into dst, accepting a short read at end of
// file once at least want_min bytes are in (the 4 KiB-rounded tail of the
// last chunk may run past EOF). -errno, or -EIO before want_min.
inline int read_span(int fd, uint8_t* dst, uint64_t want_min, uint64_t want_max, uint64_t off, std::string* err) {
    uint64_t got = 0;
    while (got < want_max) {
        const ssize_t r = pread(fd, dst + got, want_max - got, (off_t)(off + got));
        if (r < 0) {
            if (errno == EINTR) continue;
            const int code = errno;
            *err = std::string("pread: ") + strerror(code);
            return -code;
        }
        got += (uint64_t)r;
        if (r == 0 || (got >= want_min && got < want_max)) break;
    }
    if (got < want_min) {
        *err = "pread: end of file before the last record";
        return -EIO;
    }
    return 0;
}

// The cut of a span of want_max bytes (of which want_min must arrive) into at
// most kReadPieces 4 KiB-aligned pieces for parallel preads; only the last
// piece may end short (at EOF). Returns the pieces, 0 = the span is read
// serially (below 4 pages per piece).
struct ReadPiece {
    uint64_t lo;    // offset in the span
    uint64_t len;   // bytes asked for
    uint64_t need;  // bytes that must arrive
};

inline int read_pieces(uint64_t want_min, uint64_t want_max, ReadPiece out[kReadPieces]) {
    const uint64_t piece = ((want_max / kReadPieces) + kFileAlign - 1) & ~(kFileAlign - 1);
    if (want_max < 4 * kFileAlign * kReadPieces || piece == 0) return 0;
    int used = 0;
    for (uint64_t lo = 0; lo < want_max; lo += piece, ++used) {
        const uint64_t hi = lo + piece < want_max ? lo + piece : want_max;
        const bool last = hi == want_max;
        out[used].lo = lo;
        out[used].len = hi - lo;
        out[used].need = last ? (want_min > lo ? want_min - lo : 0) : hi - lo;
    }
    return used;
}

// read_span over the pieces of read_pieces in parallel on the reader pool.
inline int read_span_parallel(int fd, uint8_t* dst, uint64_t want_min, uint64_t want_max, uint64_t off,
                              std::string* err) {
    ReadPiece pc[kReadPieces];
    const int used = read_pieces(want_min, want_max, pc);
    if (!used) return read_span(fd, dst, want_min, want_max, off, err);
    int rcs[kReadPieces] = {};
    std::string errs[kReadPieces];
    std::vector<std::function<void()>> tasks;
    for (int k = 0; k < used; ++k) {
        const ReadPiece p = pc[k];
        tasks.push_back([=, &rcs, &errs] { rcs[k] = read_span(fd, dst + p.lo, p.need, p.len, off + p.lo, &errs[k]); });
    }
    ReaderPool::get().run_all(tasks);
    for (int i = 0; i < used; ++i)
        if (rcs[i]) {
            *err = errs[i];
            return rcs[i];
        }
    return 0;
}

// ---------------------------------------------------------------- pipeline
// The chunks of `pl` through two chunk buffers of at least pl.span_max bytes
// each: a reader thread fills buf[c & 1] with chunk c (waiting until the
// consumer has given that buffer back) while this thread hands the previous
// chunk to consume(records, first, k) -> int, `records` pointing at record
// `first`. Returns 0, the first non-zero code of consume, or the reader's
// error; in the last case *read_err holds its text (else it is left empty:
// consume reports its own errors). The reader thread has ended on return.
// before_read (tests): called on the reader thread before each chunk's read.
template <typename Consume>
int file_pipeline(int fd, const FilePlan& pl, uint8_t* const buf[2], Consume&& consume, std::string* read_err,
                  const std::function<void(uint64_t)>* before_read = nullptr) {
    std::mutex mu;
    std::condition_variable cv;
    int64_t ready[2] = {-1, -1};  // chunk index held by each buffer, -1 = free
    uint64_t skew[2] = {0, 0};    // record 0 of the chunk sits at buf + skew
    int read_rc = 0;
    bool stop = false;
    read_err->clear();

    std::thread reader([&] {
        for (uint64_t c = 0; c < pl.nchunks; ++c) {
            const int slot = (int)(c & 1);
            {
                std::unique_lock<std::mutex> g(mu);
                cv.wait(g, [&] { return ready[slot] < 0 || stop; });
                if (stop) return;
            }
            if (before_read) (*before_read)(c);
            const FileChunk ch = file_chunk(pl, c);
            std::string err;
            int rc = read_span_parallel(fd, buf[slot], ch.hi - ch.alo, ch.ahi - ch.alo, ch.alo, &err);
            std::unique_lock<std::mutex> g(mu);
            if (rc) {
                read_rc = rc;
                *read_err = err;
                stop = true;
                cv.notify_all();
                return;
            }
            skew[slot] = ch.skew;
            ready[slot] = (int64_t)c;
            cv.notify_all();
        }
    });

    int rc = 0;
    for (uint64_t c = 0; c < pl.nchunks && !rc; ++c) {
        const int slot = (int)(c & 1);
        uint64_t sk;
        {
            std::unique_lock<std::mutex> g(mu);
            cv.wait(g, [&] { return ready[slot] == (int64_t)c || stop; });
            if (ready[slot] != (int64_t)c) {
                rc = read_rc ? read_rc : -EIO;
                break;
            }
            sk = skew[slot];
        }
        const uint64_t first = c * pl.per;
        const uint64_t k = pl.count - first < pl.per ? pl.count - first : pl.per;
        rc = consume(buf[slot] + sk, first, k);
        std::unique_lock<std::mutex> g(mu);
        ready[slot] = -1;
        cv.notify_all();
    }
    {
        std::unique_lock<std::mutex> g(mu);
        stop = true;
        cv.notify_all();
    }
    reader.join();
    if (read_rc) return read_rc;
    return rc;
}

}  // namespace pcrc
