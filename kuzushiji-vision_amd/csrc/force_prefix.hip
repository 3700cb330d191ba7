// Forced prefixes: at a step whose chosen index cur = t + 1 lies inside the image's prefix (cur <= prefix_len[image]) the row of scores
// becomes -inf everywhere below vocab and 0 at the forced token prefix[image][cur - 1] -- HF's ForceTokensLogitsProcessor, the last node
// of the logits chain (after kzv_logits_process and kzv_lm_fuse: the prompt is subject to neither).  kzv/prefix.py: force_reference is the
// torch statement this is pinned against bit for bit.
//
// One workgroup of 256 threads per row, logits_process_kernel's shape; score_rows.h has the three ways of finding the row's image and
// step (lockstep: image r / group at the host scalar t; greedy and beam slots: image slot_image[s] at slot_t[s], s = r / group;
// by_image is accepted for symmetry with the two neighbours and changes nothing: no history is read).  The rows of an idle slot, rows
// past their prefix and columns [vocab, ld) are not written; all of that is decided before any barrier, workgroup-uniformly.
// forced_logprob (optional): the model's own opinion of the forced token, forced_logprob[image][cur], written by the first row of the
// group before the overwrite: x[f] when the row is normalised already, x[f] - lse(x) otherwise (score_rows.h: KZV_ROW_MAX_LSE, the
// reduction logits_process_kernel normalises with).  Plain stores, wave64 reductions, no atomics.
#include "score_rows.h"

#include <atomic>

namespace {

std::atomic<long long> g_launches{0};

__global__ __launch_bounds__(256) void force_prefix_kernel(const kzv_force_prefix_args p) {
    __shared__ float s_m[4], s_s[4];
    const int r = blockIdx.x, tid = threadIdx.x;
    ScoreRow at;
    if (!score_row<true>(p, r, at)) return;      // workgroup-uniform, before any barrier
    const int img = at.image, cur = at.t + 1;
    const int plen = (int)min((int64_t)p.prefix_len[img], p.ld_prefix);      // the prefix never leaves its row
    if (cur < 1 || cur > plen) return;           // past the prefix: the row stays as it is
    const int V = p.vocab;
    const int64_t f64 = p.prefix[(int64_t)img * p.ld_prefix + cur - 1];
    if (f64 < 0 || f64 >= V) return;             // (refused by the callers; never an index outside the row)
    const int f = (int)f64;
    float* __restrict__ row = p.logits + (int64_t)r * p.ld;
    constexpr int E = 8;
    if (p.forced_logprob && r % p.group == 0 && cur < p.ld_forced_logprob) {
        float val = row[f];
        if (!p.normalised) {
            float M, lse;
            KZV_ROW_MAX_LSE(E, row, V, tid, s_m, s_s, M, lse);
            val = (val - M) - lse;
        }
        if (tid == 0) p.forced_logprob[(int64_t)img * p.ld_forced_logprob + cur] = val;
        __syncthreads();                         // every read of the row is done before the first store below
    }
    for (int v = tid; v < V; v += 256) row[v] = v == f ? 0.f : -INFINITY;
}

}  // namespace

extern "C" int kzv_force_prefix(const kzv_force_prefix_args* a, void* stream) {
    if (!a) return kzv_fail(KZV_E_ARG, "force_prefix: null arguments");
    KZV_TRY_RC(score_rows_check<false>(a, "force_prefix"));
    if (!a->prefix || !a->prefix_len) return kzv_fail(KZV_E_ARG, "force_prefix: null prefix / prefix_len");
    if (a->ld_prefix < 1) return kzv_fail(KZV_E_ARG, "force_prefix: ld_prefix must be positive");
    if (a->forced_logprob && a->ld_forced_logprob < a->ld_prefix + 1)
        return kzv_fail(KZV_E_ARG, "force_prefix: forced_logprob rows of %lld columns are shorter than BOS + the %lld prefix columns", (long long)a->ld_forced_logprob, (long long)a->ld_prefix);
    hipLaunchKernelGGL(force_prefix_kernel, dim3((unsigned)a->rows), dim3(256), 0, (hipStream_t)stream, *a);
    g_launches.fetch_add(1, std::memory_order_relaxed);
    return kzv_check_launch("force_prefix");
}

// A hook for the tests, deliberately NOT declared in include/kzv.h (no part of the ABI): the kzv_force_prefix calls that reached a launch
// since the library was loaded; counted as kzv_test_logits_process_calls counts (a call made while a stream captures counts once).
extern "C" int64_t kzv_test_force_prefix_calls(void) { return (int64_t)g_launches.load(std::memory_order_relaxed); }
