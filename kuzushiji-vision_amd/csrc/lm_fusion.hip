// Shallow fusion of a character n-gram language model into one step's next-token scores, in place: x[v] += weight * lm[v]
// (kzv/lm.py: NGramLM.row states lm[], fuse_reference the fusion; this is pinned against them bit for bit; include/kzv.h: kzv_ngram_lm
// documents the tables).
//
// One workgroup of 256 threads per row, logits_process_kernel's shape, on the same histories h[0 .. n): score_rows.h has the three ways
// of finding one (lockstep, greedy slots, beam slots); the rows of an idle slot return before any barrier and stay as they are.
// Look-ups: wave k - 1 searches the sorted keys of length k for h[n - k .. n), k = 1 .. min(order - 1, n), 64 probes per round (a 65-ary
// search: the three look-ups run side by side, each in 3 - 4 dependent loads); the results (successor range, back-off; a negative range
// where nothing was found) reach the workgroup through LDS.
// Sparse phase, longest context first: threads stride over the context's successor list; whoever wins the atomicOr on the token's bit of
// the claim mask (one bit per token in LDS, 2 KiB at the 16,384-token bound) reads row[v], writes row[v] + weight * (acc + lp) and is the
// only writer of that element; a barrier between lengths makes the longest context win.  acc collects the back-offs in that order.
// Dense pass, batches of independent loads: every unclaimed v gets row[v] + weight * (acc + uni[v]).  Every element is edited once.
// The adds and the multiply are __fadd_rn / __fmul_rn and this unit is built with -ffp-contract=off, or no torch.equal could hold.
#include "score_rows.h"

#include <atomic>
#include <cmath>

namespace {

constexpr int LF_WORDS = SCORE_MAX_VOCAB / 32;   // the claim mask is 2 KiB of LDS
constexpr int LF_MAX_ORDER = 4;

std::atomic<long long> g_launches{0};

// x + weight * (acc + lp) with three roundings.  Under the library's -ffp-contract=fast even __fmul_rn / __fadd_rn (plain operators in
// HIP) are contracted into one fma, and `#pragma clang fp contract(off)` here was tried and is not honoured in that mode (nine fma left
// in the unit's assembly).  So THIS UNIT ALONE is compiled with -ffp-contract=off (the Makefile's rule for lm_fusion.o); its assembly
// then holds no fma, and nothing in it gains from contraction (tests/test_lm_gpu.py holds the kernel to torch.equal).
__device__ __forceinline__ float fused(float x, float wgt, float acc, float lp) {
    return __fadd_rn(x, __fmul_rn(wgt, __fadd_rn(acc, lp)));
}

__global__ __launch_bounds__(256) void lm_fuse_kernel(const kzv_lm_fuse_args p, const kzv_ngram_lm lm) {
    __shared__ unsigned s_claim[LF_WORDS];
    __shared__ int s_beg[LF_MAX_ORDER - 1], s_end[LF_MAX_ORDER - 1];
    __shared__ float s_bo[LF_MAX_ORDER - 1];
    const int r = blockIdx.x, tid = threadIdx.x;
    ScoreRow at;
    if (!score_row<false>(p, r, at)) return;     // workgroup-uniform, before any barrier
    const int V = p.vocab, words = (V + 31) >> 5;
    int n;
    const int64_t* __restrict__ h = score_history(p, at, n);
    const int K = min(lm.order - 1, n);
    for (int i = tid; i < words; i += 256) s_claim[i] = 0u;
    const int w = tid >> 6, lane = tid & 63;
    if (w < K) {                                 // wave w looks up the context of length k = w + 1 (wave-uniform: K <= 3 of the 4 waves)
        const int k = w + 1;
        int64_t key = 0;
        bool ok = true;
        for (int j = 0; j < k; ++j) {            // oldest token most significant
            const int64_t v = h[n - k + j];
            ok = ok && v >= 0 && v < V;
            key = key * SCORE_MAX_VOCAB + v;
        }
        int beg = -1, end = -1;
        float bo = 0.f;
        if (ok) {
            // the first index a with keys[a] >= key (n_ctx if none), a in [lo, hi]: the wave's 64 lanes probe 64 interior points per
            // round, so a table of 62,000 contexts takes 3 dependent loads and a last one over <= 64 neighbours where a binary search
            // takes 16 -- inside a decode step these loads miss the caches, and their latency was most of the node's cost
            const int64_t* __restrict__ keys = lm.keys[w];
            const int nk = lm.n_ctx[w];
            int lo = 0, hi = nk;
            while (hi - lo > 64) {               // probes lo < p_0 < .. < p_63 < hi (span >= 65: consecutive ones differ by >= 1)
                const int64_t span = hi - lo;
                const int pr = lo + (int)(((int64_t)(lane + 1) * span) / 65);
                const int c = __popcll(__ballot(keys[pr] < key));      // sorted keys: the lanes below c hold smaller keys
                const int nlo = c ? lo + (int)(((int64_t)c * span) / 65) + 1 : lo;
                const int nhi = c < 64 ? lo + (int)(((int64_t)(c + 1) * span) / 65) : hi;
                lo = nlo; hi = nhi;
            }
            const int q = lo + lane;
            const int a = lo + __popcll(__ballot(q < hi && keys[q] < key));      // (q < hi <= n_ctx: no lane reads past the table)
            if (a < nk && keys[a] == key) { beg = lm.off[w][a]; end = lm.off[w][a + 1]; bo = lm.bo[w][a]; }
        }
        if (lane == 0) { s_beg[w] = beg; s_end[w] = end; s_bo[w] = bo; }
    }
    __syncthreads();
    float* __restrict__ row = p.logits + (int64_t)r * p.ld;
    const float wgt = p.weight;
    float acc = 0.f;
    for (int k = K; k >= 1; --k) {               // workgroup-uniform: the ranges come from LDS
        const int beg = s_beg[k - 1], end = s_end[k - 1];
        if (beg < 0) continue;                   // context not found: skipped, acc unchanged
        for (int i = beg + tid; i < end; i += 256) {
            const int v = lm.succ_tok[i];
            if (v < 0 || v >= V) continue;
            const unsigned bit = 1u << (v & 31);
            if (!(atomicOr(&s_claim[v >> 5], bit) & bit)) row[v] = fused(row[v], wgt, acc, lm.succ_lp[i]);
        }
        acc = __fadd_rn(acc, s_bo[k - 1]);
        __syncthreads();                         // the longer context's claims are in place before the shorter one's are tried
    }
    constexpr int E = 8;
    const float* __restrict__ uni = lm.uni;
    for (int v0 = tid; v0 < V; v0 += 256 * E) {
        float x[E], u[E];
#pragma unroll
        for (int e = 0; e < E; ++e) { const int v = min(v0 + e * 256, V - 1); x[e] = row[v]; u[e] = uni[v]; }
#pragma unroll
        for (int e = 0; e < E; ++e) {
            const int v = v0 + e * 256;
            if (v < V && !(s_claim[v >> 5] & (1u << (v & 31)))) row[v] = fused(x[e], wgt, acc, u[e]);
        }
    }
}

}  // namespace

// what kzv_lm_fuse and kzv_stream_set_lm both refuse about the model itself; nullptr: fine
const char* kzv_ngram_lm_problem(const kzv_ngram_lm* lm, int vocab) {
    if (!lm) return "null language model";
    if (lm->order < 1 || lm->order > LF_MAX_ORDER) return "order outside 1..4";
    if (lm->vocab < 1 || lm->vocab > SCORE_MAX_VOCAB) return "the language model's vocabulary lies outside 1..16384";
    if (lm->vocab != vocab) return "the language model's vocabulary differs from the scores'";
    if (!lm->uni) return "null unigram table";
    for (int k = 0; k < lm->order - 1; ++k) {
        if (lm->n_ctx[k] < 0) return "negative context count";
        if (lm->n_ctx[k] > 0 && (!lm->keys[k] || !lm->bo[k] || !lm->off[k] || !lm->succ_tok || !lm->succ_lp)) return "null context table";
    }
    return nullptr;
}

extern "C" int kzv_lm_fuse(const kzv_lm_fuse_args* a, void* stream) {
    if (!a) return kzv_fail(KZV_E_ARG, "lm_fuse: null arguments");
    KZV_TRY_RC(score_rows_check<true>(a, "lm_fuse"));
    if (const char* why = kzv_ngram_lm_problem(a->lm, a->vocab)) return kzv_fail(KZV_E_ARG, "lm_fuse: %s", why);
    if (!std::isfinite(a->weight)) return kzv_fail(KZV_E_ARG, "lm_fuse: the weight must be finite (got %g)", (double)a->weight);
    hipLaunchKernelGGL(lm_fuse_kernel, dim3((unsigned)a->rows), dim3(256), 0, (hipStream_t)stream, *a, *a->lm);
    g_launches.fetch_add(1, std::memory_order_relaxed);
    return kzv_check_launch("lm_fuse");
}

// A hook for the tests, deliberately NOT declared in include/kzv.h (no part of the ABI): the kzv_lm_fuse calls that reached a launch since
// the library was loaded; counted as kzv_test_logits_process_calls counts (a call made while a stream captures counts once).
extern "C" int64_t kzv_test_lm_fuse_calls(void) { return (int64_t)g_launches.load(std::memory_order_relaxed); }
