// Deferred folds, as a host-only type without a HIP header: the fold launch is a function pointer, so a plain C++ program
// drives the same logic with a recording fake (tests/host/fold_queue_main.cpp).
//
// A kernel family that reduces in two phases (layernorm.hip: gamma / beta partial sums; gemm_tn256.hip: partial tiles) writes each
// launch's partials into one of REGIONS regions and folds them with a second, tiny launch.  Region 0 serves a launch whose fold follows
// at once.  While a scope is open, every launch claims a region of its own (1..REGIONS-1) and leaves its fold pending; ONE launch folds
// all of them when the outermost scope closes.
//
// Invariant: a queue is process-global and unsynchronised -- ONE host thread issues the launches of a scope, on ONE stream, and a scope
// held open defers every launch of its family in the process.  The single fold launch adds every entry to its output with a plain
// read-modify-write, so the outputs pending inside a scope are distinct: a launch whose output is already pending folds first.
#pragma once

template <class Entry, int REGIONS>
class KzvFoldQueue {
public:
    static constexpr int CAPACITY = REGIONS - 1;                    // pending entries at most: regions 1..
    typedef int (*FoldFn)(const Entry* e, int n, void* stream);     // launches ONE fold over e[0..n), n >= 1; 0 on success
    explicit KzvFoldQueue(FoldFn fold) : fold_(fold) {}
    KzvFoldQueue(const KzvFoldQueue&) = delete;

    void open() { ++depth_; }
    // the outermost close folds what is pending and returns the fold's code; an inner one returns 0
    int close(void* stream) { return --depth_ == 0 ? flush(stream) : 0; }
    // The claim rule.  Not deferring: *region = 0, nothing else happens.  Deferring: if there is no free region, or same_output(e) holds for
    // a pending e, or the caller must fold first for a reason of its own (its workspace is about to move), what is pending is folded;
    // *region = 1 + pending.  Returns the code of the fold it had to make, else 0.  The caller launches into the region and then push()es.
    template <class Same>
    int claim(Same same_output, bool must_fold_first, void* stream, int* region) {
        *region = 0;
        if (depth_ <= 0) return 0;
        bool fold = must_fold_first || n_ == CAPACITY;
        for (int i = 0; i < n_ && !fold; ++i) fold = same_output(e_[i]);
        const int rc = fold ? flush(stream) : 0;
        *region = 1 + n_;
        return rc;
    }
    void push(const Entry& e) { e_[n_++] = e; }                     // after a claim that gave a region >= 1
    // the pending entries in issue order, in one call; the list is empty afterwards whatever the fold answers
    int flush(void* stream) {
        const int n = n_;
        n_ = 0;
        return n ? fold_(e_, n, stream) : 0;
    }
    int pending() const { return n_; }

private:
    const FoldFn fold_;
    int depth_ = 0, n_ = 0;
    Entry e_[CAPACITY];
};
