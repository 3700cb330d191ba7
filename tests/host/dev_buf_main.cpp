// Drives csrc/dev_buf.h with a malloc-backed, counting allocator (no HIP, no GPU).  tests/test_dev_buf_cpu.py builds it with
// -fsanitize=address,undefined and runs it: a check that fails prints its line and exits 1, a write into a freed block or a double
// free is the sanitizer's to report.
#include "../../kuzushiji-vision_amd/csrc/dev_buf.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <thread>

#define CHECK(cond) do { if (!(cond)) { std::fprintf(stderr, "%s:%d: CHECK failed: %s\n", __FILE__, __LINE__, #cond); std::exit(1); } } while (0)

namespace {

constexpr size_t MiB = (size_t)1 << 20;
std::mutex g_mu;
std::map<void*, size_t> g_live;         // every block the allocator has handed out and not taken back
long g_allocs = 0, g_frees = 0;
size_t g_fail_above = SIZE_MAX;         // requests larger than this fail

int count_alloc(void** out, size_t bytes) {
    std::lock_guard<std::mutex> lk(g_mu);
    if (bytes > g_fail_above) { *out = nullptr; return 1; }
    void* p = std::malloc(bytes ? bytes : 1);
    if (!p) return 1;
    g_live[p] = bytes; ++g_allocs; *out = p;
    return 0;
}
void count_free(void* p) {
    std::lock_guard<std::mutex> lk(g_mu);
    CHECK(g_live.erase(p) == 1);         // a block the allocator does not hold: a double free
    ++g_frees;
    std::free(p);
}
long allocs() { std::lock_guard<std::mutex> lk(g_mu); return g_allocs; }
long frees() { std::lock_guard<std::mutex> lk(g_mu); return g_frees; }
size_t live_blocks() { std::lock_guard<std::mutex> lk(g_mu); return g_live.size(); }
bool is_live(void* p, size_t bytes) { std::lock_guard<std::mutex> lk(g_mu); auto it = g_live.find(p); return it != g_live.end() && it->second == bytes; }
// what a KzvScratch never frees is this program's to free, once the instance is gone
void free_all_live() {
    std::lock_guard<std::mutex> lk(g_mu);
    for (auto& kv : g_live) std::free(kv.first);
    g_live.clear();
}

size_t pow2_at_least(size_t n) { size_t c = MiB; while (c < n) c <<= 1; return c; }

void test_scratch() {
    const int64_t growths0 = g_kzv_scratch_growths.load();
    const long allocs0 = allocs();
    {
        KzvScratch ws(count_alloc);
        // the pointer stays for every request at or below the capacity
        char* a = (char*)ws.get(100);
        CHECK(a && ws.capacity() == MiB && allocs() == allocs0 + 1);       // the floor
        CHECK(ws.get(1) == a && ws.get(MiB) == a && ws.get(4096) == a && allocs() == allocs0 + 1);
        // growth: a new pointer, and the old block is still allocated and writable
        char* b = (char*)ws.get(MiB + 1);
        CHECK(b && b != a && ws.capacity() == 2 * MiB && allocs() == allocs0 + 2 && frees() == 0);
        CHECK(is_live(a, MiB));
        std::memset(a, 0x5a, MiB);
        std::memset(b, 0xa5, 2 * MiB);
        CHECK((unsigned char)a[MiB - 1] == 0x5a && ws.retired_blocks() == 1 && ws.retired_bytes() == MiB);
        // up, down, up again: allocations on the strict maxima only
        char* c = (char*)ws.get(5 * MiB);
        CHECK(c && c != b && ws.capacity() == 8 * MiB && allocs() == allocs0 + 3);
        CHECK(ws.get(3 * MiB) == c && ws.get(10) == c && ws.get(5 * MiB) == c && ws.get(8 * MiB) == c && allocs() == allocs0 + 3);
        char* d = (char*)ws.get(8 * MiB + 1);
        CHECK(d && d != c && ws.capacity() == 16 * MiB && allocs() == allocs0 + 4);
        CHECK(ws.get(6 * MiB) == d && allocs() == allocs0 + 4);
        std::memset(c, 1, 8 * MiB);      // retired, still writable
        CHECK(g_kzv_scratch_growths.load() - growths0 == 3);
    }
    {
        // capacity: the next power of two at or above the request, 1 MiB at least; held bytes < 2 x the live capacity after each growth
        // of a 12-step increasing sequence
        KzvScratch ws(count_alloc);
        const long a0 = allocs();
        const int64_t gr0 = g_kzv_scratch_growths.load();
        const size_t req[12] = {1, MiB / 2 + 3, MiB, MiB + 1, 3 * MiB - 7, 4 * MiB, 4 * MiB + 1, 9 * MiB, 17 * MiB, 31 * MiB, 32 * MiB + 5, 100 * MiB};
        size_t cap = 0; long expect_allocs = 0;
        for (int i = 0; i < 12; ++i) {
            char* p = (char*)ws.get(req[i]);
            CHECK(p);
            if (req[i] > cap) { cap = pow2_at_least(req[i]); ++expect_allocs; }
            CHECK(ws.capacity() == cap && cap >= req[i] && cap >= MiB && (cap & (cap - 1)) == 0 && (cap == MiB || cap / 2 < req[i]));
            CHECK(allocs() - a0 == expect_allocs);
            CHECK(ws.retired_bytes() + ws.capacity() < 2 * ws.capacity());
            CHECK(ws.retired_blocks() == (size_t)expect_allocs - 1);
            p[0] = 1; p[req[i] - 1] = 2;
        }
        // the process-wide counter: allocations minus one per instance
        CHECK(g_kzv_scratch_growths.load() - gr0 == expect_allocs - 1);
    }
    CHECK(g_kzv_scratch_growths.load() - growths0 == (allocs() - allocs0) - 2);
    {
        // an allocator failure: null, the previous pointer stays the live one, the next smaller request succeeds
        KzvScratch ws(count_alloc);
        char* a = (char*)ws.get(2 * MiB);
        CHECK(a);
        const long a0 = allocs();
        const int64_t gr0 = g_kzv_scratch_growths.load();
        g_fail_above = 3 * MiB;
        CHECK(ws.get(3 * MiB) == nullptr);           // would take a 4 MiB block
        CHECK(ws.capacity() == 2 * MiB && ws.retired_blocks() == 0 && allocs() == a0 && g_kzv_scratch_growths.load() == gr0);
        std::memset(a, 7, 2 * MiB);
        CHECK(ws.get(MiB) == a && ws.get(2 * MiB) == a);
        g_fail_above = SIZE_MAX;
        char* b = (char*)ws.get(3 * MiB);
        CHECK(b && b != a && ws.capacity() == 4 * MiB && ws.retired_blocks() == 1);
        CHECK(ws.get(SIZE_MAX) == nullptr && ws.get(3 * MiB) == b);     // no power of two holds it
    }
    {
        // a first request that fails leaves an empty workspace that still works afterwards
        KzvScratch ws(count_alloc);
        g_fail_above = 0;
        CHECK(ws.get(10) == nullptr && ws.capacity() == 0);
        g_fail_above = SIZE_MAX;
        CHECK(ws.get(10) != nullptr && ws.capacity() == MiB);
    }
    {
        // two threads, interleaved sizes: one live block, every retirement recorded
        KzvScratch ws(count_alloc);
        const long a0 = allocs();
        const int64_t gr0 = g_kzv_scratch_growths.load();
        auto worker = [&ws](int phase) {
            for (int i = 0; i < 400; ++i) {
                const size_t bytes = ((size_t)((i * 7 + phase * 3) % 40) + 1) * MiB / 2 + (size_t)i;
                char* p = (char*)ws.get(bytes);
                CHECK(p);
                p[0] = (char)i; p[bytes - 1] = (char)phase;     // valid whichever block it is: none is ever freed
            }
        };
        std::thread t0(worker, 0), t1(worker, 1);
        t0.join(); t1.join();
        const long n = allocs() - a0;
        CHECK(n >= 1 && ws.retired_blocks() == (size_t)n - 1 && g_kzv_scratch_growths.load() - gr0 == n - 1);
        CHECK(ws.capacity() == 32 * MiB);            // the largest request is just above 20 MiB
        CHECK(ws.retired_bytes() < ws.capacity());
        CHECK(ws.get(1) == ws.get(32 * MiB) && allocs() - a0 == n);
    }
    CHECK(frees() == 0);                 // a workspace never gives a block back
    free_all_live();
}

void test_dev_buf() {
    const long a0 = allocs(), f0 = frees();
    CHECK(live_blocks() == 0);
    {
        KzvDevBuf b(count_alloc, count_free);
        CHECK(!b && b.capacity() == 0 && b.as<char>() == nullptr);
        // "moved" exactly when the allocator was called; exact sizes
        CHECK(b.reserve(1000) == KzvDevBuf::MOVED && allocs() == a0 + 1 && b.capacity() == 1000 && b);
        char* p = b.as<char>();
        CHECK(is_live(p, 1000));
        std::memset(p, 1, 1000);
        CHECK(b.reserve(1000) == KzvDevBuf::KEPT && b.reserve(1) == KzvDevBuf::KEPT && b.as<char>() == p && allocs() == a0 + 1);
        // growth frees the old block exactly once
        CHECK(b.reserve(1001) == KzvDevBuf::MOVED && allocs() == a0 + 2 && frees() == f0 + 1 && b.capacity() == 1001);
        CHECK(live_blocks() == 1 && is_live(b.as<char>(), 1001));
        std::memset(b.as<char>(), 2, 1001);
        // release() then the destructor: no double free (count_free checks that it holds the block)
        b.release();
        CHECK(!b && b.capacity() == 0 && frees() == f0 + 2 && live_blocks() == 0);
        b.release();
        CHECK(frees() == f0 + 2);
    }
    CHECK(frees() == f0 + 2);
    {
        // a failed reserve: empty, not dangling; usable again
        KzvDevBuf b(count_alloc, count_free);
        CHECK(b.reserve(64) == KzvDevBuf::MOVED);
        g_fail_above = 100;
        CHECK(b.reserve(200) == KzvDevBuf::FAILED);
        CHECK(!b && b.as<char>() == nullptr && b.capacity() == 0 && live_blocks() == 0);
        CHECK(b.reserve(200) == KzvDevBuf::FAILED && !b);
        g_fail_above = SIZE_MAX;
        CHECK(b.reserve(50) == KzvDevBuf::MOVED && b.capacity() == 50);
        std::memset(b.as<char>(), 3, 50);
    }
    {
        KzvDevBuf two[2] = {KzvDevBuf(count_alloc, count_free), KzvDevBuf(count_alloc, count_free)};      // as the handle's row tables
        CHECK(two[0].reserve(10) == KzvDevBuf::MOVED && two[1].reserve(20) == KzvDevBuf::MOVED && two[0].as<int>() != two[1].as<int>());
    }
    // every alloc has its free
    CHECK(live_blocks() == 0 && allocs() - a0 == frees() - f0);
}

}  // namespace

int main() {
    test_scratch();
    test_dev_buf();
    std::printf("dev_buf: ok (%ld allocations)\n", allocs());
    return 0;
}
