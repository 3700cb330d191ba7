// Drives csrc/fold_queue.h with a recording fake fold (no HIP, no GPU), at the two capacities the library uses: 64 regions (LayerNorm
// backward) and 6 (256x256 weight gradients).  tests/test_fold_queue_cpu.py builds it with -fsanitize=address,undefined and runs it: a
// check that fails prints its line and exits 1, an entry written past the list is the sanitizer's to report.
#include "../../kuzushiji-vision_amd/csrc/fold_queue.h"
#include <cstdio>
#include <cstdlib>
#include <vector>

#define CHECK(cond) do { if (!(cond)) { std::fprintf(stderr, "%s:%d: CHECK failed: %s\n", __FILE__, __LINE__, #cond); std::exit(1); } } while (0)

namespace {

struct Entry { int out; int region; };
std::vector<std::vector<Entry>> g_calls;      // one element per fold launch: the entries it was given, in order
void* g_stream_seen = nullptr;
int g_fold_answer = 0;
int fake_fold(const Entry* e, int n, void* stream) {
    CHECK(n >= 1);
    g_calls.emplace_back(e, e + n);
    g_stream_seen = stream;
    return g_fold_answer;
}
int g_stream_tag;
void* const STREAM = &g_stream_tag;

template <int REGIONS>
struct Driver {
    KzvFoldQueue<Entry, REGIONS> q{fake_fold};
    // a launch into output `out`, as the units issue it: claim, then push when the fold is deferred
    int launch(int out, int* region, bool must_fold_first = false) {
        const int rc = q.claim([=](const Entry& e) { return e.out == out; }, must_fold_first, STREAM, region);
        if (rc == 0 && *region > 0) q.push(Entry{out, *region});
        return rc;
    }
};

template <int REGIONS>
void run() {
    constexpr int CAP = REGIONS - 1;
    static_assert(KzvFoldQueue<Entry, REGIONS>::CAPACITY == CAP, "capacity");
    int region = -1;
    g_fold_answer = 0;
    {   // not open: region 0, nothing pending, no fold -- whatever the flags say
        Driver<REGIONS> d;
        g_calls.clear();
        for (int i = 0; i < 3; ++i) { CHECK(d.launch(7, &region, i == 2) == 0 && region == 0 && d.q.pending() == 0); }
        CHECK(d.q.flush(STREAM) == 0 && g_calls.empty());
    }
    {   // open and full: regions 1.. in order; the next claim folds all of them first, in issue order and in one call, and gets region 1
        Driver<REGIONS> d;
        g_calls.clear();
        d.q.open();
        for (int i = 0; i < CAP; ++i) { CHECK(d.launch(100 + i, &region) == 0 && region == 1 + i && d.q.pending() == 1 + i); }
        CHECK(g_calls.empty());
        CHECK(d.launch(100 + CAP, &region) == 0 && region == 1 && d.q.pending() == 1);
        CHECK(g_calls.size() == 1 && (int)g_calls[0].size() == CAP && g_stream_seen == STREAM);
        for (int i = 0; i < CAP; ++i) CHECK(g_calls[0][i].out == 100 + i && g_calls[0][i].region == 1 + i);
        CHECK(d.launch(100, &region) == 0 && region == 2 && g_calls.size() == 1);      // output 100 was folded: no longer pending
        CHECK(d.q.close(STREAM) == 0 && g_calls.size() == 2 && g_calls[1].size() == 2 && g_calls[1][0].out == 100 + CAP && g_calls[1][1].out == 100);
        CHECK(d.q.pending() == 0);
        CHECK(d.launch(1, &region) == 0 && region == 0);                               // closed: back to region 0
    }
    {   // output already pending: fold first
        Driver<REGIONS> d;
        g_calls.clear();
        d.q.open();
        CHECK(d.launch(1, &region) == 0 && region == 1);
        CHECK(d.launch(2, &region) == 0 && region == 2);
        CHECK(d.launch(1, &region) == 0 && region == 1 && d.q.pending() == 1);
        CHECK(g_calls.size() == 1 && g_calls[0].size() == 2 && g_calls[0][0].out == 1 && g_calls[0][1].out == 2);
        CHECK(d.q.close(STREAM) == 0 && g_calls.size() == 2 && g_calls[1].size() == 1 && g_calls[1][0].out == 1);
    }
    {   // the must-fold-first flag: fold first; with nothing pending there is nothing to launch
        Driver<REGIONS> d;
        g_calls.clear();
        d.q.open();
        CHECK(d.launch(1, &region, true) == 0 && region == 1 && g_calls.empty());
        CHECK(d.launch(2, &region, true) == 0 && region == 1 && d.q.pending() == 1);
        CHECK(g_calls.size() == 1 && g_calls[0].size() == 1 && g_calls[0][0].out == 1);
        CHECK(d.launch(3, &region, false) == 0 && region == 2 && g_calls.size() == 1);
        CHECK(d.q.close(STREAM) == 0 && g_calls.size() == 2 && g_calls[1].size() == 2);
    }
    {   // nested open / open / close / close: one fold, at the outermost close
        Driver<REGIONS> d;
        g_calls.clear();
        d.q.open();
        CHECK(d.launch(1, &region) == 0 && region == 1);
        d.q.open();
        CHECK(d.launch(2, &region) == 0 && region == 2);
        CHECK(d.q.close(STREAM) == 0 && g_calls.empty() && d.q.pending() == 2);
        CHECK(d.launch(3, &region) == 0 && region == 3);                               // still deferring
        CHECK(d.q.close(STREAM) == 0 && g_calls.size() == 1 && g_calls[0].size() == 3 && d.q.pending() == 0);
        for (int i = 0; i < 3; ++i) CHECK(g_calls[0][i].out == 1 + i && g_calls[0][i].region == 1 + i);
        // a fold forced inside the nested scope is one call too, and the outer close folds the rest
        g_calls.clear();
        d.q.open(); d.q.open();
        for (int i = 0; i < CAP + 1; ++i) CHECK(d.launch(10 + i, &region) == 0 && region == (i < CAP ? 1 + i : 1));
        CHECK(g_calls.size() == 1 && (int)g_calls[0].size() == CAP);
        CHECK(d.q.close(STREAM) == 0 && g_calls.size() == 1);
        CHECK(d.q.close(STREAM) == 0 && g_calls.size() == 2 && g_calls[1].size() == 1 && g_calls[1][0].out == 10 + CAP);
    }
    {   // close with nothing pending: no fold
        Driver<REGIONS> d;
        g_calls.clear();
        d.q.open();
        CHECK(d.q.close(STREAM) == 0 && g_calls.empty());
        d.q.open(); d.q.open();
        CHECK(d.q.close(STREAM) == 0 && d.q.close(STREAM) == 0 && g_calls.empty());
    }
    {   // a fold that fails: the claim reports it, the list is empty afterwards; close() reports a failing fold too
        Driver<REGIONS> d;
        g_calls.clear();
        d.q.open();
        for (int i = 0; i < CAP; ++i) CHECK(d.launch(i, &region) == 0);
        g_fold_answer = -2;
        CHECK(d.launch(CAP, &region) == -2 && d.q.pending() == 0 && g_calls.size() == 1 && (int)g_calls[0].size() == CAP);
        CHECK(d.q.close(STREAM) == 0 && g_calls.size() == 1);                          // nothing left to fold
        g_fold_answer = 0;
        d.q.open();
        CHECK(d.launch(1, &region) == 0 && region == 1);
        g_fold_answer = -2;
        CHECK(d.launch(1, &region) == -2 && d.q.pending() == 0);                       // through "already pending"
        g_fold_answer = 0;
        CHECK(d.launch(1, &region) == 0 && region == 1);
        g_fold_answer = -2;
        CHECK(d.launch(2, &region, true) == -2 && d.q.pending() == 0);                 // through the flag
        g_fold_answer = 0;
        CHECK(d.launch(5, &region) == 0 && d.launch(6, &region) == 0 && region == 2);
        g_fold_answer = -2;
        CHECK(d.q.close(STREAM) == -2 && d.q.pending() == 0 && g_calls.size() == 4 && g_calls[3].size() == 2);
        g_fold_answer = 0;
        CHECK(d.launch(5, &region) == 0 && region == 0);                               // the scope did close
    }
}

}  // namespace

int main() {
    run<64>();      // LN_REGIONS: 63 pending
    run<6>();       // TN_REGIONS: 5 pending
    std::printf("fold_queue: ok\n");
    return 0;
}
