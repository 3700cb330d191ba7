// The two ways this library owns device memory, as host-only types without a HIP header: the allocator is a pair of
// function pointers, so a plain C++ program drives the same logic with malloc (tests/host/dev_buf_main.cpp).
//   KzvDevBuf   a buffer of the model handle: exact size, freed when it has to grow and with the handle.  reserve() reports a pointer
//               that moved, and the caller drops the captured graphs that hold the old one.
//   KzvScratch  a process workspace: a pointer it has handed out stays valid for the life of the process, for the captured graphs and
//               the kernels in flight that hold it.  Growth neither waits for the device nor frees anything.
#pragma once
#include <atomic>
#include <cstddef>
#include <cstdint>
#include <mutex>
#include <vector>

typedef int (*KzvAllocFn)(void** out, size_t bytes);       // 0 on success
typedef void (*KzvFreeFn)(void* p);
int kzv_dev_alloc(void** out, size_t bytes);               // host.cpp: hipMalloc / hipFree, the default pair
void kzv_dev_free(void* p);

class KzvDevBuf {
public:
    enum Result { FAILED = -1, KEPT = 0, MOVED = 1 };
    explicit KzvDevBuf(KzvAllocFn a = kzv_dev_alloc, KzvFreeFn f = kzv_dev_free) : alloc_(a), free_(f) {}
    KzvDevBuf(const KzvDevBuf&) = delete;                  // (which deletes the assignment too: the members below are const)
    ~KzvDevBuf() { release(); }
    // KEPT: the block already holds `bytes`.  MOVED: the old block was freed and exactly `bytes` allocated.  FAILED: the buffer is empty.
    Result reserve(size_t bytes) {
        if (p_ && bytes <= cap_) return KEPT;
        release();
        if (alloc_(&p_, bytes) != 0 || !p_) { p_ = nullptr; return FAILED; }
        cap_ = bytes;
        return MOVED;
    }
    void release() { if (p_) free_(p_); p_ = nullptr; cap_ = 0; }
    template <class T> T* as() const { return (T*)p_; }
    size_t capacity() const { return cap_; }
    explicit operator bool() const { return p_ != nullptr; }

private:
    void* p_ = nullptr; size_t cap_ = 0;
    const KzvAllocFn alloc_; const KzvFreeFn free_;
};

// how often any KzvScratch of the process has moved to a new block (kzv_scratch_growths)
inline std::atomic<int64_t> g_kzv_scratch_growths{0};

class KzvScratch {
public:
    explicit KzvScratch(KzvAllocFn a = kzv_dev_alloc) : alloc_(a) {}        // (not copyable: the mutex)
    // At least `bytes`, or nullptr when the allocation fails (the previous block stays the live one).  The capacity is the next power
    // of two >= bytes, 1 MiB at least: a process grows a workspace ~30 times at most, and the blocks left behind (retired, never
    // freed: no destructor touches the device at exit either) are distinct smaller powers of two, together less than the live one.
    void* get(size_t bytes) {
        std::lock_guard<std::mutex> lk(mu_);
        if (p_ && bytes <= cap_) return p_;
        if (bytes > SIZE_MAX / 2) return nullptr;
        size_t cap = (size_t)1 << 20;
        while (cap < bytes) cap <<= 1;
        void* q = nullptr;
        if (alloc_(&q, cap) != 0 || !q) return nullptr;
        if (p_) { retired_.push_back(p_); retired_bytes_ += cap_; ++g_kzv_scratch_growths; }
        p_ = q; cap_ = cap;
        return p_;
    }
    size_t capacity() const { std::lock_guard<std::mutex> lk(mu_); return cap_; }
    size_t retired_bytes() const { std::lock_guard<std::mutex> lk(mu_); return retired_bytes_; }
    size_t retired_blocks() const { std::lock_guard<std::mutex> lk(mu_); return retired_.size(); }

private:
    mutable std::mutex mu_;
    void* p_ = nullptr; size_t cap_ = 0, retired_bytes_ = 0;
    std::vector<void*> retired_;
    const KzvAllocFn alloc_;
};
