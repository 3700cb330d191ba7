// The k best columns of fp32 logits rows and their log-softmax values -- the alternatives of a recognised character:
//   kzv_token_topk   over [rows, ld] logits (HF: output_scores=True, scores[t].log_softmax(-1).topk(k))
//   kzv_stream_topk  over the slots' rows of one slot-refill step, written to alt[image][t + 1][0..k) while slot_image / slot_t still
//                    describe the step (before kzv_stream_update seats the next images)
// One wave per row, four rows per 256-thread workgroup, token_scores_kernel's launch shape and its two paths (16 bytes per lane where the
// rows are 16-byte aligned, then the tail by column; by column throughout otherwise).  A lane scans its columns in ASCENDING order with
// unconditional loads and keeps (a) row_scan.h's running (max, sum exp) and (b) a list of its TOPK_DEPTH = 8 best (value, column) pairs,
// sorted best first, in registers: a column enters only if it ranks before the list's last entry (one compare), then sinks into place by
// seven compare-swaps with compile-time indices.  The row's k best are all among the 64 lists' entries, so the wave extracts them in k
// rounds: a 6-step xor-shuffle arg-max over the list heads, the winning lane pops its head.  The order is by descending logit, ties by
// ascending column -- the FIRST arg-max rule of token_scores_kernel / stream_select_kernel, so entry 0 is their top-1; -inf logits are
// legal, rank last (ties by column) and get log-probability -inf; empty list entries (value -inf, column ROW_NO_COL) rank after every
// real column and come out as id -1 / -inf where vocab < k.  NaN never enters a list (every compare against it is false): ids stay in
// [-1, vocab).  No LDS, no atomics, a fixed order everywhere: the result is bit-reproducible.
#include "row_scan.h"
#include "../../include/kzv.h"
#include "kzv_host.h"

namespace {

constexpr int TOPK_DEPTH = 8;

struct LaneTopk {
    float v[TOPK_DEPTH]; int c[TOPK_DEPTH];
    __device__ __forceinline__ LaneTopk() {
#pragma unroll
        for (int j = 0; j < TOPK_DEPTH; ++j) { v[j] = -INFINITY; c[j] = ROW_NO_COL; }
    }
    __device__ __forceinline__ void take(float x, int col) {
        if (!row_before(x, col, v[TOPK_DEPTH - 1], c[TOPK_DEPTH - 1])) return;
        v[TOPK_DEPTH - 1] = x; c[TOPK_DEPTH - 1] = col;
#pragma unroll
        for (int j = TOPK_DEPTH - 1; j > 0; --j) {
            const bool up = row_before(v[j], c[j], v[j - 1], c[j - 1]);
            const float tv = v[j]; const int tc = c[j];
            v[j] = up ? v[j - 1] : tv; c[j] = up ? c[j - 1] : tc;
            v[j - 1] = up ? tv : v[j - 1]; c[j - 1] = up ? tc : c[j - 1];
        }
    }
    __device__ __forceinline__ void pop() {
#pragma unroll
        for (int j = 0; j < TOPK_DEPTH - 1; ++j) { v[j] = v[j + 1]; c[j] = c[j + 1]; }
        v[TOPK_DEPTH - 1] = -INFINITY; c[TOPK_DEPTH - 1] = ROW_NO_COL;
    }
};

// the whole wave works on the row `lr`; lanes 0 .. k - 1 then store entry `lane` to ids / logprob
__device__ __forceinline__ void row_topk(const float* __restrict__ lr, int vocab, int vec, int k, int lane, int32_t* __restrict__ ids,
                                         float* __restrict__ logprob) {
    RowScan st;
    LaneTopk tk;
    const int nv = vec ? vocab >> 2 : 0;                     // float4 pieces (rows 16-byte aligned), then the tail by column
    for (int i = lane; i < nv; i += 64) {
        const float4 x = ((const float4*)lr)[i];
        st.take(x.x, 4 * i); st.take(x.y, 4 * i + 1); st.take(x.z, 4 * i + 2); st.take(x.w, 4 * i + 3);
        tk.take(x.x, 4 * i); tk.take(x.y, 4 * i + 1); tk.take(x.z, 4 * i + 2); tk.take(x.w, 4 * i + 3);
    }
    for (int j = 4 * nv + lane; j < vocab; j += 64) {
        const float x = lr[j];
        st.take(x, j); tk.take(x, j);
    }
    float mx = st.mx;
    int arg = st.arg;
    wave_first_argmax(mx, arg);
    const float lse = wave_lse(st, mx);
    float my_v = -INFINITY; int my_c = ROW_NO_COL;           // entry `lane` of the result
    for (int r = 0; r < k; ++r) {
        float bv = tk.v[0]; int bc = tk.c[0];
        wave_first_argmax(bv, bc);
        if (lane == r) { my_v = bv; my_c = bc; }
        if (bc != ROW_NO_COL && tk.c[0] == bc) tk.pop();      // columns are unique: exactly one lane
    }
    if (lane < k) {
        const bool none = my_c == ROW_NO_COL;
        ids[lane] = none ? -1 : my_c;
        logprob[lane] = (none || my_v == -INFINITY) ? -INFINITY : my_v - lse;      // (an all -inf row has lse = -inf)
    }
}

__global__ __launch_bounds__(256) void token_topk_kernel(const float* __restrict__ logits, int64_t ld, int rows, int vocab, int vec, int k,
                                                         int32_t* __restrict__ ids, float* __restrict__ logprob) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;                                 // wave-uniform; no barrier follows
    row_topk(logits + (int64_t)row * ld, vocab, vec, k, lane, ids + (int64_t)row * k, logprob + (int64_t)row * k);
}

// slot `row` holds image slot_image[row] (< 0: idle) at step slot_t[row]: stream_select_kernel's conditions for writing out_ids[img][t + 1]
__global__ __launch_bounds__(256) void stream_topk_kernel(const float* __restrict__ logits, int64_t ld, int slots, int vocab, int vec, int k,
                                                          const int* __restrict__ slot_image, const int* __restrict__ slot_t, int n_images, int max_len,
                                                          int32_t* __restrict__ alt_ids, float* __restrict__ alt_logprob, int64_t ld_alt) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= slots) return;                                // wave-uniform, as are the next two; no barrier follows
    const int img = slot_image[row];
    if (img < 0 || img >= n_images) return;
    const int t = slot_t[row];
    if (t < 0 || t + 1 >= max_len) return;
    const int64_t at = (int64_t)img * ld_alt + (int64_t)(t + 1) * k;
    row_topk(logits + (int64_t)row * ld, vocab, vec, k, lane, alt_ids + at, alt_logprob + at);
}

int topk_args(const char* who, const float* logits, int64_t ld, int vocab, int k, const int32_t* ids, const float* logprob) {
    if (!logits || !ids || !logprob) return kzv_fail(KZV_E_ARG, "%s: null operand", who);
    if (k < 1 || k > TOPK_DEPTH) return kzv_fail(KZV_E_ARG, "%s: k must be in 1..%d (got %d)", who, TOPK_DEPTH, k);
    if (vocab < 1 || ld < vocab) return kzv_fail(KZV_E_ARG, "%s: need vocab >= 1 and ld >= vocab (got vocab %d, ld %lld)", who, vocab, (long long)ld);
    return KZV_OK;
}

int topk_vec(const float* logits, int64_t ld) { return (ld % 4 == 0 && ((uintptr_t)logits & 15) == 0) ? 1 : 0; }

}  // namespace

extern "C" int kzv_token_topk(const float* logits, int64_t ld, int64_t rows, int vocab, int k, int32_t* ids, float* logprob, void* stream) {
    KZV_TRY_RC(topk_args("token_topk", logits, ld, vocab, k, ids, logprob));
    if (rows < 1 || rows >= (1ll << 31)) return kzv_fail(KZV_E_ARG, "token_topk: rows must be in 1..2^31 - 1 (got %lld)", (long long)rows);
    hipLaunchKernelGGL(token_topk_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, (hipStream_t)stream, logits, ld, (int)rows, vocab,
                       topk_vec(logits, ld), k, ids, logprob);
    return kzv_check_launch("token_topk");
}

extern "C" int kzv_stream_topk(const kzv_stream_state* st, const float* d_logits, int64_t ld, int k, int32_t* d_alt_ids, float* d_alt_logprob,
                               int64_t ld_alt, void* stream) {
    if (!st) return kzv_fail(KZV_E_ARG, "stream_topk: null state");
    if (!st->slot_image || !st->slot_t) return kzv_fail(KZV_E_ARG, "stream_topk: null state array");
    if (st->slots < 1 || st->n_images < 1 || st->max_len < 2) return kzv_fail(KZV_E_ARG, "stream_topk: slots and images must be positive, max_len >= 2");
    KZV_TRY_RC(topk_args("stream_topk", d_logits, ld, st->vocab, k, d_alt_ids, d_alt_logprob));
    if (ld_alt < (int64_t)st->max_len * k) return kzv_fail(KZV_E_ARG, "stream_topk: ld_alt %lld < max_len * k = %lld", (long long)ld_alt, (long long)st->max_len * k);
    hipLaunchKernelGGL(stream_topk_kernel, dim3((unsigned)((st->slots + 3) / 4)), dim3(256), 0, (hipStream_t)stream, d_logits, ld, st->slots, st->vocab,
                       topk_vec(d_logits, ld), k, st->slot_image, st->slot_t, st->n_images, st->max_len, d_alt_ids, d_alt_logprob, ld_alt);
    return kzv_check_launch("stream_topk");
}
