// Generation controls on one step's next-token scores, in place (kzv/controls.py::process_reference is the readable statement this is
// pinned against): transformers' RepetitionPenaltyLogitsProcessor, NoRepeatNGramLogitsProcessor, MinLengthLogitsProcessor and
// SuppressTokensLogitsProcessor, in the order GenerationMixin._get_logits_processor builds them.  The last three only write -inf and the
// penalty maps -inf to -inf, so the order is immaterial for the result: the kernel collects two vocabulary bitmasks first and edits every
// element once.
//
// One workgroup of 256 threads per row (stream_select_kernel's shape).  The row's token history h[0 .. n) is read where it lies
// (score_rows.h: score_row / score_history, shared with the chain's other two nodes):
//   lockstep      row r: ids[r][0 .. t + 1), t a host scalar
//   greedy slots  slot s = r: ids[slot_image[s]][0 .. slot_t[s] + 1) (out_ids of the wave)
//   beam slots    row r of slot s = r / group: ids[r][0 .. slot_t[s] + 1) (run_seq of the wave)
// with the step index of the slot cases read from device memory, so that one captured graph serves every step.  A slot with
// slot_image < 0 is idle: its rows return before any barrier and stay as they are.
// The sparse part runs in LDS: "seen" (tokens of the history: the penalty's targets) and "banned" (n-gram continuations, EOS below the
// minimum length, the caller's suppress mask) hold one bit per token, 2 KiB each at the 16,384-token bound, filled with LDS atomics by
// threads striding over the history -- thread i compares the g - 1 tokens h[i ..] with the history's tail.  Then one dense pass in batches
// of independent loads (beam_topk_kernel's remedy for a round trip per element).  With `normalise` a first phase takes the row's maximum
// and sum of exponentials in the order of beam_topk_kernel's first phase (token_search.hip): thread tid owns tokens tid + 256 e; the WAVE's
// maximum first (wave_max of the threads' maxima), each thread's exponentials summed against it in ascending e, wave_sum, then the four
// waves' (max, sum) merged under the row maximum.  The dense pass writes (x - max) - log(sum), that kernel's own expression.
#include "score_rows.h"

#include <atomic>

namespace {

constexpr int LP_WORDS = SCORE_MAX_VOCAB / 32;   // the two masks are 2 * 2 KiB of LDS
constexpr int LP_MAX_NGRAM = 8;

std::atomic<long long> g_launches{0};

template <bool NORM>
__global__ __launch_bounds__(256) void logits_process_kernel(const kzv_logits_process_args p) {
    __shared__ unsigned s_seen[LP_WORDS], s_ban[LP_WORDS];
    __shared__ float s_m[4], s_s[4];
    const int r = blockIdx.x, tid = threadIdx.x;
    ScoreRow at;
    if (!score_row<false>(p, r, at)) return;     // workgroup-uniform, before any barrier
    const int V = p.vocab, words = (V + 31) >> 5;
    int n;
    const int64_t* __restrict__ h = score_history(p, at, n);
    const int g = p.no_repeat_ngram_size;
    const float pen = p.repetition_penalty;
    const bool penalise = pen != 1.f;
    for (int i = tid; i < words; i += 256) { s_seen[i] = 0u; s_ban[i] = p.suppress_mask ? p.suppress_mask[i] : 0u; }
    __syncthreads();
    if (penalise || g == 1) {                    // g = 1 bans every token of the history
        for (int i = tid; i < n; i += 256) {
            const int64_t v = h[i];
            if (v < 0 || v >= V) continue;
            if (penalise) atomicOr(&s_seen[v >> 5], 1u << (v & 31));
            if (g == 1) atomicOr(&s_ban[v >> 5], 1u << (v & 31));
        }
    }
    if (g >= 2 && n + 1 >= g) {                  // every i in 0 .. n - g whose g - 1 tokens equal the history's last g - 1
        const int64_t* tail = h + (n - g + 1);
        for (int i = tid; i + g <= n; i += 256) {
            bool same = true;
            for (int j = 0; j < g - 1; ++j) same = same && h[i + j] == tail[j];
            const int64_t v = h[i + g - 1];
            if (same && v >= 0 && v < V) atomicOr(&s_ban[v >> 5], 1u << (v & 31));
        }
    }
    if (tid == 0 && n < p.min_length && p.eos_id >= 0 && p.eos_id < V) atomicOr(&s_ban[p.eos_id >> 5], 1u << (p.eos_id & 31));
    __syncthreads();
    float* __restrict__ row = p.logits + (int64_t)r * p.ld;
    constexpr int E = 8;
    float M = 0.f, lse = 0.f;
    if (NORM) KZV_ROW_MAX_LSE(E, row, V, tid, s_m, s_s, M, lse);      // its barrier: every read of the first phase is done before the first store below
    for (int v0 = tid; v0 < V; v0 += 256 * E) {
        float x[E];
#pragma unroll
        for (int e = 0; e < E; ++e) x[e] = row[min(v0 + e * 256, V - 1)];
#pragma unroll
        for (int e = 0; e < E; ++e) {
            const int v = v0 + e * 256;
            if (v < V) {
                float y = NORM ? (x[e] - M) - lse : x[e];
                const unsigned bit = 1u << (v & 31);
                if (penalise && (s_seen[v >> 5] & bit)) y = y < 0.f ? y * pen : __fdiv_rn(y, pen);      // a true division: == torch
                if (s_ban[v >> 5] & bit) y = -INFINITY;
                row[v] = y;
            }
        }
    }
}

}  // namespace

extern "C" int kzv_logits_process(const kzv_logits_process_args* a, void* stream) {
    if (!a) return kzv_fail(KZV_E_ARG, "logits_process: null arguments");
    KZV_TRY_RC(score_rows_check<true>(a, "logits_process"));
    if (a->no_repeat_ngram_size < 0 || a->no_repeat_ngram_size > LP_MAX_NGRAM)
        return kzv_fail(KZV_E_ARG, "logits_process: no_repeat_ngram_size %d outside 0..%d", a->no_repeat_ngram_size, LP_MAX_NGRAM);
    if (!(a->repetition_penalty > 0.f)) return kzv_fail(KZV_E_ARG, "logits_process: repetition_penalty must be positive (got %g)", (double)a->repetition_penalty);
    if (a->min_length < 0) return kzv_fail(KZV_E_ARG, "logits_process: min_length must not be negative");
    if (a->min_length > 0 && (a->eos_id < 0 || a->eos_id >= a->vocab)) return kzv_fail(KZV_E_ARG, "logits_process: EOS %d outside the vocabulary", a->eos_id);
    if (a->normalise) hipLaunchKernelGGL(logits_process_kernel<true>, dim3((unsigned)a->rows), dim3(256), 0, (hipStream_t)stream, *a);
    else hipLaunchKernelGGL(logits_process_kernel<false>, dim3((unsigned)a->rows), dim3(256), 0, (hipStream_t)stream, *a);
    g_launches.fetch_add(1, std::memory_order_relaxed);
    return kzv_check_launch("logits_process");
}

// A hook for the tests, deliberately NOT declared in include/kzv.h (no part of the ABI): the kzv_logits_process calls that reached a launch
// since the library was loaded.  A call made while a stream captures counts once, the graph's replays do not -- every wave captures its own
// step (kzv_stream_begin drops the last wave's graph), so "the counter stands still across a call" means no step of it held the node.
extern "C" int64_t kzv_test_logits_process_calls(void) { return (int64_t)g_launches.load(std::memory_order_relaxed); }
