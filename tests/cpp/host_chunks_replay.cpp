// host_chunks_replay.cpp -- the host-side chunking of the host-memory pipeline
// and of photon_crc32c_file_strided (photonlibos_amd/csrc/host_chunks.h) on
// the CPU, stand-alone; also built with -fsanitize=address,undefined and with
// -fsanitize=thread. Linked with crc32c_cpu.cpp: crc32c_sw plays the GPU
// pipeline in the consumer of file_pipeline.
//
//   1. stage_plan / stage_chunk: the chunks cover [0, count) once and in
//      order, slot == i % 3, and a chunk fits its span and the allocation;
//   2. file_plan / file_chunk: alignment, skew, the buffer bound, and every
//      record of every chunk inside the span read;
//   3. read_pieces: the parallel cut of a chunk's read;
//   4. file_pipeline on real temporary files with end of file at every edge
//      (O_RDONLY, and O_DIRECT where the filesystem takes it);
//   5. file_pipeline over 1, 2, 3, 5 and 8 chunks as it is, with a slow
//      consumer (the reader waits for a free buffer) and with a slow reader,
//      with a failing consumer, with a read error in a later chunk, and two
//      pipelines at once over the shared ReaderPool.
// Every chunk buffer is heap memory of exactly span_max bytes. An alarm ends
// the program if a pipeline deadlocks.
//
// Usage: host_chunks_replay [directory for the temporary files]. Prints
//   host_chunks_replay: <n> stage plans, <n> file geometries, <n> piece cuts, <n> file reads,
//       <n> pipelines, o_direct <ok|refused>, <n> mismatches        (one line)
#ifndef _GNU_SOURCE
#define _GNU_SOURCE
#endif
#include <fcntl.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <unistd.h>

#include <atomic>
#include <chrono>
#include <string>
#include <thread>
#include <vector>

#include <photon/common/checksum/crc32c.h>

#include "host_chunks.h"

using namespace pcrc;

namespace {

uint64_t g_bad = 0;
std::mutex g_bad_mu;

void bad(const char* fmt, ...) {
    std::lock_guard<std::mutex> lk(g_bad_mu);
    if (g_bad++ < 20) {
        va_list ap;
        va_start(ap, fmt);
        vfprintf(stderr, fmt, ap);
        va_end(ap);
        fputc('\n', stderr);
    }
}

#define CHECK(cond, ...) \
    do {                 \
        if (!(cond)) bad(__VA_ARGS__); \
    } while (0)

// ------------------------------------------------------------ 1. staging plan
uint64_t check_stage_plans() {
    const uint64_t nb[] = {1,     255,   256,    257,    511,     512,       513,           4104,        65535,
                           65536, 65537, 65544,  100000, 600000,  1ull << 20, (1ull << 20) + 1, kStageBytes - 256,
                           kStageBytes - 255, kStageBytes};
    const uint64_t spans[] = {kStageMinSpan, kStageMinSpan + 256, 1ull << 20, (1ull << 20) + 768, 16ull << 20, kStageBytes};
    uint64_t plans = 0;
    for (uint64_t nbytes : nb)
        for (uint64_t span : spans) {
            const uint64_t pitch = (nbytes + 255) / 256 * 256;
            const uint64_t per = span / pitch ? span / pitch : 1;
            for (uint64_t m : {0, 1, 2, 3, 4, 7})
                for (int d = -1; d <= 1; ++d) {
                    if (m * per + d + 1 == 0) continue;  // -1
                    const uint64_t count = m * per + d;
                    const StagePlan pl = stage_plan(nbytes, count, span);
                    ++plans;
                    CHECK(pl.pitch == pitch && pl.per_chunk == per && pl.count == count,
                          "stage_plan(%llu, %llu, %llu): pitch %llu per_chunk %llu", (unsigned long long)nbytes,
                          (unsigned long long)count, (unsigned long long)span, (unsigned long long)pl.pitch,
                          (unsigned long long)pl.per_chunk);
                    CHECK(pl.nchunks == (count + per - 1) / per, "stage_plan(%llu, %llu, %llu): %llu chunks",
                          (unsigned long long)nbytes, (unsigned long long)count, (unsigned long long)span,
                          (unsigned long long)pl.nchunks);
                    uint64_t next = 0;
                    for (uint64_t i = 0; i < pl.nchunks; ++i) {
                        const StageChunk c = stage_chunk(pl, i);
                        const bool fits = c.k * pitch <= span || (per == 1 && pitch > span && c.k == 1);
                        CHECK(c.first == next && c.k >= 1 && c.k <= per && c.first + c.k <= count &&
                                  (c.k == per || i + 1 == pl.nchunks) && c.slot == (int)(i % 3) && fits &&
                                  c.k * pitch <= kStageBytes,
                              "stage_chunk(%llu, %llu, %llu) chunk %llu: first %llu k %llu slot %d",
                              (unsigned long long)nbytes, (unsigned long long)count, (unsigned long long)span,
                              (unsigned long long)i, (unsigned long long)c.first, (unsigned long long)c.k, c.slot);
                        next = c.first + c.k;
                    }
                    CHECK(next == count, "stage_plan(%llu, %llu, %llu): covers %llu", (unsigned long long)nbytes,
                          (unsigned long long)count, (unsigned long long)span, (unsigned long long)next);
                }
        }
    for (uint64_t b : {uint64_t(0), kStageMinSpan, kStageMinSpan + 256, kStageBytes})
        CHECK(stage_span_valid(b), "stage span %llu refused", (unsigned long long)b);
    for (uint64_t b : {uint64_t(1), uint64_t(256), kStageMinSpan - 256, kStageMinSpan + 1, kStageBytes + 256, ~uint64_t(0)})
        CHECK(!stage_span_valid(b), "stage span %llu accepted", (unsigned long long)b);
    return plans;
}

// ------------------------------------------------------------ 2. file geometry
uint64_t check_file_geometry() {
    uint64_t geoms = 0;
    for (uint64_t chunk : {uint64_t(4096), uint64_t(65536), uint64_t(262144)}) {
        const uint64_t strides[] = {7, 100, 4096, chunk - 1, chunk, chunk + 1, 3 * chunk + 5};
        for (uint64_t offset : {0, 1, 4095, 4096, 4097})
            for (uint64_t stride : strides) {
                const uint64_t per0 = chunk / stride ? chunk / stride : 1;
                for (uint64_t nbytes : {uint64_t(1), stride / 2 ? stride / 2 : 1, stride > 1 ? stride - 1 : 1, stride})
                    for (uint64_t m : {1, 2, 3, 5})
                        for (int d = -1; d <= 1; ++d) {
                            const uint64_t count = m * per0 + d;
                            if (!count) continue;
                            const FilePlan pl = file_plan(offset, stride, nbytes, count, chunk);
                            ++geoms;
                            const uint64_t per = per0 < count ? per0 : count;
                            CHECK(pl.per == per && pl.nchunks == (count + per - 1) / per &&
                                      pl.span_max == (per - 1) * stride + nbytes + 2 * kFileAlign,
                                  "file_plan(%llu, %llu, %llu, %llu, %llu): per %llu chunks %llu span_max %llu",
                                  (unsigned long long)offset, (unsigned long long)stride, (unsigned long long)nbytes,
                                  (unsigned long long)count, (unsigned long long)chunk, (unsigned long long)pl.per,
                                  (unsigned long long)pl.nchunks, (unsigned long long)pl.span_max);
                            uint64_t next = 0, wrong = 0;
                            for (uint64_t c = 0; c < pl.nchunks; ++c) {
                                const FileChunk ch = file_chunk(pl, c);
                                const bool ok =
                                    ch.first == next && ch.k >= 1 && ch.k <= per && (ch.k == per || c + 1 == pl.nchunks) &&
                                    ch.lo == offset + ch.first * stride && ch.hi == ch.lo + (ch.k - 1) * stride + nbytes &&
                                    ch.alo <= ch.lo && ch.ahi >= ch.hi && ch.alo % kFileAlign == 0 &&
                                    ch.ahi % kFileAlign == 0 && ch.skew == ch.lo - ch.alo && ch.skew < kFileAlign &&
                                    ch.ahi - ch.hi < kFileAlign && ch.ahi - ch.alo <= pl.span_max;
                                wrong += !ok;
                                for (uint64_t r = 0; r < ch.k; ++r) {
                                    const uint64_t at = ch.skew + r * stride;  // in the buffer
                                    wrong += !(at >= ch.skew && at + nbytes <= ch.hi - ch.alo && at + nbytes <= ch.ahi - ch.alo &&
                                               ch.alo + at == offset + (ch.first + r) * stride);
                                }
                                next = ch.first + ch.k;
                            }
                            CHECK(!wrong && next == count, "file_chunk(%llu, %llu, %llu, %llu, %llu): %llu wrong, covers %llu",
                                  (unsigned long long)offset, (unsigned long long)stride, (unsigned long long)nbytes,
                                  (unsigned long long)count, (unsigned long long)chunk, (unsigned long long)wrong,
                                  (unsigned long long)next);
                        }
            }
    }
    for (uint64_t b : {uint64_t(0), uint64_t(4096), uint64_t(65536), kFileChunk})
        CHECK(file_chunk_valid(b), "file chunk %llu refused", (unsigned long long)b);
    for (uint64_t b : {uint64_t(1), uint64_t(4095), uint64_t(4097), kFileChunk + 4096, ~uint64_t(0)})
        CHECK(!file_chunk_valid(b), "file chunk %llu accepted", (unsigned long long)b);
    return geoms;
}

// ------------------------------------------------------------ 3. piece cut
uint64_t check_piece_cuts() {
    uint64_t cuts = 0;
    std::vector<uint64_t> spans;
    for (uint64_t s = kFileAlign; s <= (2ull << 20); s += kFileAlign) spans.push_back(s);
    for (uint64_t s : {kFileChunk, kFileChunk + kFileAlign, kFileChunk + 2 * kFileAlign, 3 * kFileChunk + 5 * kFileAlign})
        spans.push_back(s);
    for (uint64_t want_max : spans)
        for (uint64_t short_by : {uint64_t(0), uint64_t(1), uint64_t(2048), kFileAlign - 1}) {
            const uint64_t want_min = want_max - short_by;
            ReadPiece pc[kReadPieces];
            for (ReadPiece& p : pc) p = ReadPiece{~0ull, ~0ull, ~0ull};
            const int used = read_pieces(want_min, want_max, pc);
            ++cuts;
            const bool serial = want_max < 4 * kFileAlign * kReadPieces;
            CHECK((used == 0) == serial && used <= kReadPieces, "read_pieces(%llu, %llu): %d pieces",
                  (unsigned long long)want_min, (unsigned long long)want_max, used);
            uint64_t next = 0;
            bool ok = true;
            for (int i = 0; i < used && i < kReadPieces; ++i) {
                const bool last = i + 1 == used;
                ok = ok && pc[i].lo == next && pc[i].lo % kFileAlign == 0 && pc[i].len > 0 &&
                     (last ? pc[i].need == want_min - pc[i].lo && pc[i].need > 0 && pc[i].need <= pc[i].len
                           : pc[i].need == pc[i].len);
                next = pc[i].lo + pc[i].len;
            }
            CHECK(ok && (used == 0 || next == want_max), "read_pieces(%llu, %llu): bad cut, covers %llu",
                  (unsigned long long)want_min, (unsigned long long)want_max, (unsigned long long)next);
        }
    return cuts;
}

// ------------------------------------------------------------ files
uint64_t mix64(uint64_t z) {
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// Non-repeating bytes: the same bytes at another file offset give another CRC.
std::vector<uint8_t> stream(uint64_t seed, uint64_t n) {
    std::vector<uint8_t> v((n + 7) / 8 * 8);
    for (uint64_t k = 0; k < v.size() / 8; ++k) {
        const uint64_t w = mix64(seed + (k + 1) * 0x9E3779B97F4A7C15ull);
        memcpy(&v[8 * k], &w, 8);
    }
    v.resize(n);
    return v;
}

std::string g_dir = "/tmp";

struct TempFile {
    std::string path;
    explicit TempFile(const uint8_t* p, uint64_t n) {
        path = g_dir + "/host_chunks_XXXXXX";
        const int fd = mkstemp(&path[0]);
        if (fd < 0) {
            perror("mkstemp");
            exit(2);
        }
        for (uint64_t done = 0; done < n;) {
            const ssize_t w = write(fd, p + done, n - done);
            if (w <= 0) {
                perror("write");
                exit(2);
            }
            done += (uint64_t)w;
        }
        close(fd);
    }
    ~TempFile() { unlink(path.c_str()); }
};

// The file as one plain read() loop sees it.
std::vector<uint8_t> plain_read(const std::string& path) {
    std::vector<uint8_t> v;
    const int fd = open(path.c_str(), O_RDONLY);
    if (fd < 0) {
        perror("open");
        exit(2);
    }
    uint8_t tmp[65536];
    for (;;) {
        const ssize_t r = read(fd, tmp, sizeof tmp);
        if (r < 0) {
            perror("read");
            exit(2);
        }
        if (!r) break;
        v.insert(v.end(), tmp, tmp + r);
    }
    close(fd);
    return v;
}

struct Shape {
    uint64_t offset, stride, nbytes, count, chunk;
    uint64_t end() const { return offset + (count - 1) * stride + nbytes; }
};

enum Pace { kPlain, kSlowConsumer, kSlowReader };
const uint32_t kUntouched = 0xA5A5A5A5u;
const uint32_t kSeed = 0x1234;

struct Run {
    int rc = 0;
    std::string err;
    std::vector<uint32_t> out;
    uint64_t ahead = 0;  // reads begun before the buffer's previous chunk was consumed
};

// One file_pipeline call over `fd` with heap buffers of exactly span_max
// bytes (4 KiB-aligned as the library's pinned buffers are, for O_DIRECT);
// the consumer fails with fail_code in chunk fail_at (-1: never).
Run run_pipeline(int fd, const Shape& s, Pace pace, int64_t fail_at = -1, int fail_code = 0) {
    const FilePlan pl = file_plan(s.offset, s.stride, s.nbytes, s.count, s.chunk);
    uint8_t* buf[2];
    for (uint8_t*& b : buf) {
        void* p = nullptr;
        if (posix_memalign(&p, kFileAlign, pl.span_max)) exit(2);
        b = static_cast<uint8_t*>(p);
        memset(b, 0xEE, pl.span_max);
    }
    Run r;
    r.out.assign(s.count, kUntouched);
    std::atomic<uint64_t> consumed{0}, ahead{0};
    const std::function<void(uint64_t)> before_read = [&](uint64_t c) {
        // buffer c & 1 is free only once chunk c - 2 has been consumed
        if (c >= 2 && consumed.load() + 1 < c) ++ahead;
        if (pace == kSlowReader) std::this_thread::sleep_for(std::chrono::milliseconds(2));
    };
    r.rc = file_pipeline(
        fd, pl, buf,
        [&](const uint8_t* rec, uint64_t first, uint64_t k) {
            if (pace == kSlowConsumer) std::this_thread::sleep_for(std::chrono::milliseconds(2));
            const uint64_t c = first / pl.per;
            if ((int64_t)c == fail_at) {
                ++consumed;
                return fail_code;
            }
            for (uint64_t i = 0; i < k; ++i) r.out[first + i] = crc32c_sw(rec + i * s.stride, s.nbytes, kSeed);
            ++consumed;
            return 0;
        },
        &r.err, &before_read);
    r.ahead = ahead.load();
    free(buf[0]);
    free(buf[1]);
    return r;
}

// out[0 .. upto) against the CRCs of the same bytes of `img`; the rest untouched.
void check_records(const char* what, const Run& r, const Shape& s, const std::vector<uint8_t>& img, uint64_t upto,
                   uint64_t untouched_from) {
    uint64_t wrong = 0, first_wrong = 0;
    for (uint64_t i = 0; i < upto; ++i) {
        const uint32_t want = crc32c_sw(&img[s.offset + i * s.stride], s.nbytes, kSeed);
        if (r.out[i] != want && !wrong++) first_wrong = i;
    }
    for (uint64_t i = untouched_from; i < s.count; ++i)
        if (r.out[i] != kUntouched && !wrong++) first_wrong = i;
    CHECK(!wrong, "%s: %llu wrong records, first %llu", what, (unsigned long long)wrong, (unsigned long long)first_wrong);
    CHECK(!r.ahead, "%s: %llu reads into a buffer still in use", what, (unsigned long long)r.ahead);
}

void expect_ok(const char* what, const std::string& path, const Shape& s, const std::vector<uint8_t>& img, Pace pace,
               int flags = O_RDONLY) {
    const int fd = open(path.c_str(), flags);
    if (fd < 0) {
        perror("open");
        exit(2);
    }
    const Run r = run_pipeline(fd, s, pace);
    close(fd);
    CHECK(r.rc == 0 && r.err.empty(), "%s: rc %d (%s)", what, r.rc, r.err.c_str());
    check_records(what, r, s, img, s.count, s.count);
}

// A read error: -EIO with the end-of-file text. The first chunk that the file
// does not hold fails; every chunk before it was read before the reader got
// there and is consumed, nothing is written from it on.
void expect_eio(const char* what, const std::string& path, const Shape& s, const std::vector<uint8_t>& img, Pace pace) {
    const int fd = open(path.c_str(), O_RDONLY);
    if (fd < 0) {
        perror("open");
        exit(2);
    }
    const Run r = run_pipeline(fd, s, pace);
    close(fd);
    CHECK(r.rc == -EIO && r.err == "pread: end of file before the last record", "%s: rc %d (%s)", what, r.rc,
          r.err.c_str());
    const FilePlan pl = file_plan(s.offset, s.stride, s.nbytes, s.count, s.chunk);
    uint64_t bad_chunk = 0;
    while (bad_chunk < pl.nchunks && file_chunk(pl, bad_chunk).hi <= img.size()) ++bad_chunk;
    if (bad_chunk == pl.nchunks) exit(3);
    check_records(what, r, s, img, bad_chunk * pl.per, bad_chunk * pl.per);
}

const uint64_t kFileBytes = (3ull << 20) + 1234;

uint64_t check_file_reads(bool* o_direct_ok) {
    uint64_t reads = 0;
    const std::vector<uint8_t> data = stream(0xF11E5, kFileBytes);
    // serial reads (64 KiB chunks) and the parallel cut (256 KiB chunks)
    for (uint64_t chunk : {uint64_t(65536), uint64_t(262144)}) {
        const Shape aligned{4096, 8192, 4096, 128, chunk};  // ends on a 4 KiB multiple
        const Shape ragged{777, 65552, 65536, 21, chunk};   // ends inside a page
        for (const Shape& s : {aligned, ragged}) {
            const FilePlan pl = file_plan(s.offset, s.stride, s.nbytes, s.count, s.chunk);
            const FileChunk last = file_chunk(pl, pl.nchunks - 1);
            const FileChunk second = file_chunk(pl, 1);
            if (pl.nchunks < 3) exit(3);
            struct Case {
                const char* what;
                uint64_t len;
                bool ok;
            };
            std::vector<Case> cases = {
                {"eof at the last record's end", s.end(), true},
                {"eof one byte short", s.end() - 1, false},
                {"eof at the second chunk's first byte", second.lo, false},
                {"eof at the second chunk's first page", second.alo, false},
                {"the whole file", kFileBytes, true},
            };
            if (s.end() % kFileAlign) cases.push_back({"eof inside the rounded tail", s.end() + 100, true});
            ReadPiece pc[kReadPieces];
            const int used = read_pieces(last.hi - last.alo, last.ahi - last.alo, pc);
            if ((used != 0) != (chunk == 262144)) exit(3);
            if (used)  // inside the second piece of the last chunk's cut
                cases.push_back({"eof inside an earlier piece", last.alo + pc[1].lo + pc[1].len / 2, false});
            for (const Case& c : cases) {
                TempFile f(data.data(), c.len);
                const std::vector<uint8_t> img = plain_read(f.path);
                if (img.size() != c.len || memcmp(img.data(), data.data(), c.len)) exit(2);
                for (Pace pace : {kPlain, kSlowConsumer, kSlowReader}) {
                    ++reads;
                    if (c.ok)
                        expect_ok(c.what, f.path, s, img, pace);
                    else
                        expect_eio(c.what, f.path, s, img, pace);
                }
            }
        }
    }
    // O_DIRECT: the aligned spans are legal (4 KiB-aligned offset, length and buffer).
    {
        TempFile f(data.data(), kFileBytes);
        const Shape s{777, 65552, 65536, 40, 262144};
        const int fd = open(f.path.c_str(), O_RDONLY | O_DIRECT);
        *o_direct_ok = false;
        if (fd >= 0) {
            const Run r = run_pipeline(fd, s, kPlain);
            close(fd);
            if (r.rc == 0) {
                *o_direct_ok = true;
                check_records("O_DIRECT", r, s, data, s.count, s.count);
            } else {
                CHECK(r.rc == -EINVAL, "O_DIRECT: rc %d (%s)", r.rc, r.err.c_str());  // the filesystem's rules
            }
        }
        ++reads;
    }
    return reads;
}

// ------------------------------------------------------------ 5. pipelines
uint64_t check_pipelines() {
    uint64_t pipes = 0;
    const std::vector<uint8_t> data = stream(0xC0FFEE, kFileBytes);
    TempFile f(data.data(), kFileBytes);
    const std::vector<uint8_t> img = plain_read(f.path);
    if (img != data) exit(2);
    // per = 3 records (parallel cut) and per = 16 records (serial reads)
    for (uint64_t n : {1, 2, 3, 5, 8})
        for (int ragged = 0; ragged < 2; ++ragged) {
            const Shape a{777, 65552, 65536, 3 * n - ragged, 262144};
            const Shape b{4097, 4096, 4000, 16 * n - ragged, 65536};
            for (const Shape& s : {a, b}) {
                if (file_plan(s.offset, s.stride, s.nbytes, s.count, s.chunk).nchunks != n) exit(3);
                for (Pace pace : {kPlain, kSlowConsumer, kSlowReader}) {
                    ++pipes;
                    expect_ok("pipeline", f.path, s, img, pace);
                }
            }
        }
    // The consumer fails in chunk 0, in a middle chunk, in the last chunk.
    {
        const Shape s{777, 65552, 65536, 15, 262144};  // 5 chunks of 3
        for (int64_t at : {0, 2, 4})
            for (Pace pace : {kPlain, kSlowConsumer, kSlowReader}) {
                const int fd = open(f.path.c_str(), O_RDONLY);
                const Run r = run_pipeline(fd, s, pace, at, -71 - (int)at);
                close(fd);
                ++pipes;
                CHECK(r.rc == -71 - (int)at && r.err.empty(), "consumer fails in chunk %lld: rc %d (%s)", (long long)at,
                      r.rc, r.err.c_str());
                check_records("consumer fails", r, s, img, 3 * (uint64_t)at, 3 * (uint64_t)at);
            }
    }
    // A read error in a later chunk (end of file inside chunk 3 of 5) while the
    // consumer works on, or waits for, an earlier one.
    {
        const Shape s{777, 65552, 65536, 15, 262144};
        const FileChunk ch = file_chunk(file_plan(s.offset, s.stride, s.nbytes, s.count, s.chunk), 3);
        TempFile cut(data.data(), ch.lo + 70000);
        const std::vector<uint8_t> cut_img = plain_read(cut.path);
        for (Pace pace : {kPlain, kSlowConsumer, kSlowReader}) {
            ++pipes;
            expect_eio("read error in chunk 3", cut.path, s, cut_img, pace);
        }
    }
    // Two pipelines at once over the shared ReaderPool.
    for (int round = 0; round < 3; ++round) {
        const Shape sa{5, 32784, 32768, 64, 262144};  // 10 chunks of 7
        const Shape sb{123, 100, 37, 20000, 262144};  // 8 chunks of 2621
        std::thread ta([&] { expect_ok("concurrent a", f.path, sa, img, kPlain); });
        std::thread tb([&] { expect_ok("concurrent b", f.path, sb, img, round == 1 ? kSlowConsumer : kPlain); });
        ta.join();
        tb.join();
        pipes += 2;
    }
    return pipes;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc > 1) g_dir = argv[1];
    alarm(120);  // a deadlocked pipeline ends the program (SIGALRM) instead of hanging it
    const uint64_t plans = check_stage_plans();
    const uint64_t geoms = check_file_geometry();
    const uint64_t cuts = check_piece_cuts();
    bool o_direct_ok = false;
    const uint64_t reads = check_file_reads(&o_direct_ok);
    const uint64_t pipes = check_pipelines();
    printf("host_chunks_replay: %llu stage plans, %llu file geometries, %llu piece cuts, %llu file reads, "
           "%llu pipelines, o_direct %s, %llu mismatches\n",
           (unsigned long long)plans, (unsigned long long)geoms, (unsigned long long)cuts, (unsigned long long)reads,
           (unsigned long long)pipes, o_direct_ok ? "ok" : "refused", (unsigned long long)g_bad);
    return g_bad ? 1 : 0;
}
