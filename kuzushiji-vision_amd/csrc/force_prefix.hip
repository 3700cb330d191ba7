// Forced prefixes: at a step whose chosen index cur = t + 1 lies inside the image's prefix (cur <= prefix_len[image]) the row of scores
// becomes -inf everywhere below vocab and 0 at the forced token prefix[image][cur - 1] -- HF's ForceTokensLogitsProcessor, the last node
// of the logits chain (after kzv_logits_process and kzv_lm_fuse: the prompt is subject to neither).  kzv/prefix.py: force_reference is the
// torch statement this is pinned against bit for bit.
//
// One workgroup of 256 threads per row, logits_process_kernel's shape and its three ways of finding the row's step:
//   lockstep      row r of image r / group at the host scalar t
//   greedy slots  slot s = r (group 1): image slot_image[s] at slot_t[s]
//   beam slots    row r of slot s = r / group: image slot_image[s] at slot_t[s]
// (by_image is accepted for symmetry with the two neighbours and changes nothing: no history is read).  The rows of an idle slot, rows
// past their prefix and columns [vocab, ld) are not written; all of that is decided before any barrier, workgroup-uniformly.
// forced_logprob (optional): the model's own opinion of the forced token, forced_logprob[image][cur], written by the first row of the
// group before the overwrite: x[f] when the row is normalised already, x[f] - lse(x) otherwise (maximum, then the sum against it per wave,
// the four waves merged through LDS: logits_process_kernel's order).  Plain stores, wave64 reductions, no atomics.
#include "kzv_common.h"
#include "../../include/kzv.h"
#include "kzv_host.h"

#include <atomic>

namespace {

constexpr int FP_MAX_VOCAB = 64 * 256;           // the bound of the chain's other two nodes

std::atomic<long long> g_launches{0};

__global__ __launch_bounds__(256) void force_prefix_kernel(const kzv_force_prefix_args p) {
    __shared__ float s_m[4], s_s[4];
    const int r = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    int t = p.t;
    int img = r / p.group;
    if (p.slot_image) {                          // workgroup-uniform, before any barrier
        img = p.slot_image[img];
        if (img < 0 || img >= p.n_images) return;
        t = p.slot_t[r / p.group];
    }
    const int cur = t + 1;
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
            float lm = -INFINITY;
            for (int v0 = tid; v0 < V; v0 += 256 * E) {
                float x[E];
#pragma unroll
                for (int e = 0; e < E; ++e) x[e] = row[min(v0 + e * 256, V - 1)];
#pragma unroll
                for (int e = 0; e < E; ++e) if (v0 + e * 256 < V) lm = fmaxf(lm, x[e]);
            }
            const float wm = wave_max(lm);
            float ls = 0.f;
            for (int v0 = tid; v0 < V; v0 += 256 * E) {
                float x[E];
#pragma unroll
                for (int e = 0; e < E; ++e) x[e] = row[min(v0 + e * 256, V - 1)];
#pragma unroll
                for (int e = 0; e < E; ++e) ls += (v0 + e * 256 < V && x[e] != -INFINITY) ? expf(x[e] - wm) : 0.f;
            }
            ls = wave_sum(ls);
            if (lane == 0) { s_m[w] = wm; s_s[w] = ls; }
            __syncthreads();
            const float M = fmaxf(fmaxf(s_m[0], s_m[1]), fmaxf(s_m[2], s_m[3]));
            float S = 0.f;
#pragma unroll
            for (int q = 0; q < 4; ++q) S += (s_m[q] == -INFINITY) ? 0.f : s_s[q] * expf(s_m[q] - M);
            val = (val - M) - logf(S);
        }
        if (tid == 0) p.forced_logprob[(int64_t)img * p.ld_forced_logprob + cur] = val;
        __syncthreads();                         // every read of the row is done before the first store below
    }
    for (int v = tid; v < V; v += 256) row[v] = v == f ? 0.f : -INFINITY;
}

}  // namespace

extern "C" int kzv_force_prefix(const kzv_force_prefix_args* a, void* stream) {
    if (!a) return kzv_fail(KZV_E_ARG, "force_prefix: null arguments");
    if (!a->logits) return kzv_fail(KZV_E_ARG, "force_prefix: null logits");
    if (!a->prefix || !a->prefix_len) return kzv_fail(KZV_E_ARG, "force_prefix: null prefix / prefix_len");
    if (a->rows < 1) return kzv_fail(KZV_E_ARG, "force_prefix: rows must be positive (got %d)", a->rows);
    if (a->vocab < 1 || a->vocab > FP_MAX_VOCAB) return kzv_fail(KZV_E_ARG, "force_prefix: vocab %d outside 1..%d", a->vocab, FP_MAX_VOCAB);
    if (a->ld < a->vocab) return kzv_fail(KZV_E_ARG, "force_prefix: ld %lld < vocab %d", (long long)a->ld, a->vocab);
    if (a->ld_prefix < 1) return kzv_fail(KZV_E_ARG, "force_prefix: ld_prefix must be positive");
    if (a->group < 1 || a->rows % a->group) return kzv_fail(KZV_E_ARG, "force_prefix: %d rows are no multiple of %d rows per image", a->rows, a->group);
    if (a->forced_logprob && a->ld_forced_logprob < a->ld_prefix + 1)
        return kzv_fail(KZV_E_ARG, "force_prefix: forced_logprob rows of %lld columns are shorter than BOS + the %lld prefix columns", (long long)a->ld_forced_logprob, (long long)a->ld_prefix);
    if ((a->slot_image == nullptr) != (a->slot_t == nullptr)) return kzv_fail(KZV_E_ARG, "force_prefix: slot_image and slot_t go together");
    if (a->slot_image) {
        if (a->n_images < 1) return kzv_fail(KZV_E_ARG, "force_prefix: n_images must be positive");
    } else if (a->t < 0) {
        return kzv_fail(KZV_E_ARG, "force_prefix: step %d is negative", a->t);
    }
    hipLaunchKernelGGL(force_prefix_kernel, dim3((unsigned)a->rows), dim3(256), 0, (hipStream_t)stream, *a);
    g_launches.fetch_add(1, std::memory_order_relaxed);
    return kzv_check_launch("force_prefix");
}

// A hook for the tests, deliberately NOT declared in include/kzv.h (no part of the ABI): the kzv_force_prefix calls that reached a launch
// since the library was loaded; counted as kzv_test_logits_process_calls counts (a call made while a stream captures counts once).
extern "C" int64_t kzv_test_force_prefix_calls(void) { return (int64_t)g_launches.load(std::memory_order_relaxed); }
