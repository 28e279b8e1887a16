// The task-to-part search and the plan replay of the packed parts calls
// (photonlibos_amd/csrc/parts_packed_plan.h) stand-alone on the host, meant
// for -fsanitize=address,undefined: every array is heap memory of exactly its
// size and the replay's workspace is never cleared.
//
//   search  packed_owner over first[] arrays made from piece counts: runs of
//           zero-count parts (front, middle, end), a single part, counts of 1
//           only, one count of 2^33 among small ones. Every task (or, for the
//           large count, the tasks around every boundary and a stride of the
//           rest) must land in the part whose [first[i], first[i+1]) holds it.
//   replay  packed_replay over parts of mixed lengths and source offsets, more
//           than one plan tile of them: first[] is the running sum of
//           parts_count, owner[] matches a linear walk, and the tasks'
//           pieces tile every part in order; with too small a total the report
//           says overflow and no owner word is written.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <memory>
#include <vector>

#include "parts_packed_plan.h"

using namespace pcrc;

static int failures = 0;
#define CHECK(c, ...)                     \
    do {                                  \
        if (!(c)) {                       \
            if (++failures < 20) {        \
                printf("FAIL %s: ", #c);  \
                printf(__VA_ARGS__);      \
                printf("\n");             \
            }                             \
        }                                 \
    } while (0)

static uint64_t checked = 0;

static void check_task(const uint64_t* first, uint64_t nparts, uint64_t t, const char* what) {
    const uint64_t i = packed_owner(first, nparts, t);
    CHECK(i < nparts, "%s: task %llu -> part %llu of %llu", what, (unsigned long long)t, (unsigned long long)i,
          (unsigned long long)nparts);
    if (i < nparts)
        CHECK(first[i] <= t && t < first[i + 1], "%s: task %llu -> part %llu [%llu, %llu)", what,
              (unsigned long long)t, (unsigned long long)i, (unsigned long long)first[i],
              (unsigned long long)first[i + 1]);
    ++checked;
}

static void search_case(const std::vector<uint64_t>& counts, const char* what) {
    const uint64_t nparts = counts.size();
    std::unique_ptr<uint64_t[]> first(new uint64_t[nparts + 1]);
    uint64_t at = 0;
    for (uint64_t i = 0; i < nparts; ++i) {
        first[i] = at;
        at = packed_add(at, counts[i]);
    }
    first[nparts] = at;
    const uint64_t T = at;
    if (T <= (1u << 16)) {
        for (uint64_t t = 0; t < T; ++t) check_task(first.get(), nparts, t, what);
        return;
    }
    for (uint64_t i = 0; i <= nparts; ++i)  // around every boundary
        for (int d = -2; d <= 2; ++d) {
            const uint64_t t = first[i] + (uint64_t)(int64_t)d;
            if (t < T) check_task(first.get(), nparts, t, what);
        }
    for (uint64_t t = 0; t < T; t += T / 4099 + 1) check_task(first.get(), nparts, t, what);
}

static void replay_case(uint64_t nparts, uint64_t piece, uint64_t max_bytes, bool overflow, uint64_t word) {
    std::unique_ptr<uint64_t[]> addr(new uint64_t[nparts]), len(new uint64_t[nparts]);
    uint64_t x = 0x9E3779B97F4A7C15ull * (nparts + piece), total = 0, want_tasks = 0;
    static const uint64_t kLens[] = {0, 1, 17, 4095, 4096, 4097, 8192, 12289, 70001, 0, 0, 300000};
    static const uint64_t kOffs[] = {0, 1, 5, 2048, 4081, 4095};
    for (uint64_t i = 0; i < nparts; ++i) {
        x ^= x << 13, x ^= x >> 7, x ^= x << 17;
        len[i] = kLens[x % 12];
        addr[i] = (1ull << 32) + (i << 20) + kOffs[(x >> 8) % 6];
        const PackedSum s = packed_part(addr[i], len[i], max_bytes, piece);
        total += s.bytes;
        want_tasks += s.tasks;
    }
    const uint64_t max_total = overflow ? total / 2 : total;
    const uint64_t slots = packed_slots(nparts, max_total, piece);
    const PackedLayout l = packed_layout(nparts, slots, word);
    std::unique_ptr<uint8_t[]> raw(new uint8_t[l.bytes]);  // operator new: 16-byte aligned
    memset(raw.get(), 0x5A, l.bytes);
    uint64_t report[4];
    packed_replay(addr.get(), len.get(), nparts, max_bytes, piece, slots, word, raw.get(), report);
    const uint64_t* first = reinterpret_cast<const uint64_t*>(raw.get() + l.first);
    const uint32_t* owner = reinterpret_cast<const uint32_t*>(raw.get() + l.owner);
    CHECK(report[1] == want_tasks && report[2] == total && report[3] == slots, "report of %llu parts",
          (unsigned long long)nparts);
    CHECK(report[0] == (want_tasks > slots ? 1u : 0u), "overflow flag");
    CHECK(first[nparts] == want_tasks, "first[nparts]");
    if (!overflow) CHECK(want_tasks <= slots, "T %llu > C %llu", (unsigned long long)want_tasks,
                         (unsigned long long)slots);
    uint64_t at = 0;
    for (uint64_t i = 0; i < nparts; ++i) {
        CHECK(first[i] == at, "first[%llu]", (unsigned long long)i);
        const uint64_t n = len[i] < max_bytes ? len[i] : max_bytes;
        const uint64_t count = parts_count(addr[i], n, piece);
        if (!report[0]) {
            uint64_t pos = 0;
            for (uint64_t j = 0; j < count; ++j) {  // the part's tasks tile it in order
                const uint64_t t = at + j;
                const uint64_t o = packed_owner_clamp(owner[t], nparts);
                CHECK(o == i, "owner[%llu] = %llu, want %llu", (unsigned long long)t, (unsigned long long)o,
                      (unsigned long long)i);
                const PartsPiece pc = packed_piece(addr[o], n, piece, first[o], t);
                CHECK(pc.off == pos && pc.len > 0, "task %llu of part %llu", (unsigned long long)t,
                      (unsigned long long)i);
                pos += pc.len;
                ++checked;
            }
            CHECK(pos == n, "part %llu: %llu of %llu bytes", (unsigned long long)i, (unsigned long long)pos,
                  (unsigned long long)n);
            // a task index that is not the part's gives an empty piece, never one outside [0, n)
            const PartsPiece behind = packed_piece(addr[i], n, piece, at, at + count + (count ? 0 : 1));
            CHECK(behind.len == 0, "piece behind the end of part %llu", (unsigned long long)i);
            CHECK(packed_piece(addr[i], n, piece, at + 1, at).len == 0, "first task above the task");
            CHECK(packed_piece(addr[i], n, piece, 0, ~0ull).len == 0, "a piece index that wraps");
        }
        at += count;
    }
    if (report[0])  // nothing of owner[] was written
        for (uint64_t t = 0; t < slots; ++t) CHECK(owner[t] == 0x5A5A5A5Au, "owner[%llu] written", (unsigned long long)t);
}

int main() {
    search_case({5}, "a single part");
    search_case({1}, "a single part of one piece");
    search_case(std::vector<uint64_t>(3000, 1), "counts of 1 only");
    {
        std::vector<uint64_t> c = {0, 0, 0, 3, 0, 1, 0, 0, 0, 0, 7, 1, 1, 0, 0, 2, 0, 0, 0};
        search_case(c, "runs of zero-count parts");
        std::vector<uint64_t> many;
        for (int r = 0; r < 300; ++r) many.insert(many.end(), c.begin(), c.end());
        search_case(many, "runs of zero-count parts, repeated");
    }
    search_case({0, 2, 1ull << 33, 0, 0, 1, 9, 0}, "one count of 2^33");
    search_case({1ull << 33}, "one count of 2^33 alone");
    {
        std::vector<uint64_t> c(70000, 1);
        c[12345] = 1ull << 33;
        c[12346] = 0;
        search_case(c, "one count of 2^33 among 70,000 parts");
    }
    for (uint64_t word : {4, 8})
        for (uint64_t piece : {4096ull, 65536ull})
            for (uint64_t nparts : {1ull, 2ull, 255ull, 1024ull, 1025ull, 2500ull})
                for (uint64_t cap : {~0ull, 10000ull, 8192ull, 8191ull, 0ull}) {
                    replay_case(nparts, piece, cap, false, word);
                    replay_case(nparts, piece, cap, true, word);
                }
    // saturating sums
    CHECK(packed_add(~0ull, 1) == ~0ull && packed_add(1ull << 63, 1ull << 63) == ~0ull && packed_add(2, 3) == 5,
          "packed_add");
    printf("%llu tasks checked, %d mismatches\n", (unsigned long long)checked, failures);
    return failures ? 1 : 0;
}
