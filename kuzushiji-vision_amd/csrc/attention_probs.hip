// What a recognised line's decoder knows beyond its token ids, read back from the activations a teacher-forced pass leaves behind:
//   kzv_attn_probs    head-averaged attention probabilities  map[b, q, k] = (1 / heads) * sum_h exp(q_h . k_h * 64^-0.5 - LSE[b, h, q])
//                     (the probabilities BEFORE dropout; HF: output_attentions=True -> cross_attentions[layer].mean(1) in eval mode),
//                     their centroid on the patch grid, their peak and its key, and the row sum as a health value (~ 1)
//   kzv_token_scores  per-token log-probabilities and the arg-max token from fp32 logits rows
// Inputs follow kzv_attn_args: Q [B * Sq, ldq], K [B * Sk, ldk] in bf16 with head h at column h * 64, LSE fp32 [B, heads, Sq] in
// natural log exactly as kzv_attn_fwd / kzv_attn_stream_fwd write it.  Mode 0, head_dim 64, Sq in 1..288, Sk in 1..4,097.
//
// attn_probs_kernel: a workgroup owns 64 query rows of one image, a wave one tile of 16 of them (waves never synchronise: no LDS, no
// barrier).  The orientation is attention.hip's: S^T = K . Q^T with the KEY on the accumulator rows and the query on the lane column,
// 16x16x32 bf16 MFMA, operands straight from memory (a wave's K fragments are 16-byte pieces of rows the other waves and the next
// head read too: they come from L1 / L2; per image K is Sk * heads * 128 bytes).  The wave sweeps the keys in blocks of 64; for each
// block it loops over the heads and adds exp2(S * sc - lse) into ONE set of accumulators, so the head sum never leaves registers, in
// head order.  Each lane then folds its 16 values of the block (four keys of four tiles, ascending) into the running state of its
// query row: sum P * (k / grid_w), sum P * (k % grid_w), sum P, the largest P and its first key.  After the sweep the four lanes of a
// query (l15, + 16, + 32, + 48) are combined by two xor shuffles -- a fixed order, so every output is bit-reproducible; there are no
// atomics and nothing whose size grows with Sk.  Rows past Sq and keys past Sk are loaded as zeros and their probabilities are
// replaced by 0 before anything accumulates (no -inf anywhere: exp2 never sees a NaN).
// Rounding points: q, k bf16 (exact products, fp32 accumulation in the MFMA); s * sc - lse, exp2, the head sum and the row state fp32.
#include "attention_common.h"
#include "row_scan.h"

namespace {

constexpr int PKB = 64;                 // keys per block of the sweep

struct ProbsP {
    const bf16_t* Q; const bf16_t* K; const float* LSE;
    float* map; float* pos; int* peak;
    int64_t ldq, ldk, ld_map;
    int B, heads, Sq, Sk, grid_w, nqb;   // nqb: 64-query blocks per image
    float inv_heads; int map_vec;        // map_vec: rows of map are 16-byte aligned (float4 stores)
};

// the better of two (value, key) candidates: the larger value, the smaller key among equals (the FIRST arg-max)
__device__ __forceinline__ void peak_fold(float& v, int& k, float ov, int ok) {
    if (ov > v || (ov == v && ok < k)) { v = ov; k = ok; }
}

__global__ __launch_bounds__(256) void attn_probs_kernel(const ProbsP p) {
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, g = lane >> 4, l15 = lane & 15;
    const int b = blockIdx.x / p.nqb, qblk = blockIdx.x - b * p.nqb;
    const int q0 = (qblk * 4 + w) * 16;
    if (q0 >= p.Sq) return;                                  // wave-uniform; no barrier follows
    const int q = q0 + l15;
    const bool qok = q < p.Sq;
    const bf16x8 zero8 = (bf16x8){0, 0, 0, 0, 0, 0, 0, 0};
    const bf16_t* qrow = p.Q + ((int64_t)b * p.Sq + (qok ? q : 0)) * p.ldq + 8 * g;
    const bf16_t* Kb = p.K + (int64_t)b * p.Sk * p.ldk + 8 * g;
    const float* lse_b = p.LSE + (int64_t)b * p.heads * p.Sq + (qok ? q : 0);
    const float sc = 0.125f * LOG2E;                         // 64^-0.5 in fp32, log2 units
    float sum_r = 0.f, sum_c = 0.f, sum_p = 0.f, best = -1.f;
    int best_k = 0;
    const int nkb = (p.Sk + PKB - 1) / PKB;
    for (int kb = 0; kb < nkb; ++kb) {
        f32x4 acc[4];
#pragma unroll
        for (int kt = 0; kt < 4; ++kt) acc[kt] = (f32x4){0.f, 0.f, 0.f, 0.f};
        for (int h = 0; h < p.heads; ++h) {
            bf16x8 qf[2], kf[4][2];
#pragma unroll
            for (int i = 0; i < 2; ++i) qf[i] = qok ? *(const bf16x8*)(qrow + h * 64 + 32 * i) : zero8;
            const float lse2 = qok ? lse_b[(int64_t)h * p.Sq] * LOG2E : 0.f;
#pragma unroll
            for (int kt = 0; kt < 4; ++kt) {
                const int key = kb * PKB + kt * 16 + l15;    // this lane's row of the A operand
#pragma unroll
                for (int i = 0; i < 2; ++i)
                    kf[kt][i] = key < p.Sk ? *(const bf16x8*)(Kb + (int64_t)key * p.ldk + h * 64 + 32 * i) : zero8;
            }
#pragma unroll
            for (int kt = 0; kt < 4; ++kt) {
                f32x4 s = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int i = 0; i < 2; ++i) s = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf[kt][i], qf[i], s, 0, 0, 0);
#pragma unroll
                for (int r = 0; r < 4; ++r) {                // key kb * 64 + kt * 16 + 4 g + r of query l15
                    const float pr = __builtin_amdgcn_exp2f(fmaf(s[r], sc, -lse2));
                    const bool ok = qok && kb * PKB + kt * 16 + 4 * g + r < p.Sk;
                    acc[kt][r] += ok ? pr : 0.f;
                }
            }
        }
#pragma unroll
        for (int kt = 0; kt < 4; ++kt) {
            const int k0 = kb * PKB + kt * 16 + 4 * g;
            if (k0 >= p.Sk) continue;
            float v[4];
            int row = k0 / p.grid_w, col = k0 - row * p.grid_w;          // one division per four keys, then a counter
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                v[r] = acc[kt][r] * p.inv_heads;
                if (k0 + r < p.Sk) {                         // (past Sk the value is an exact 0: it must not enter the peak's tie either)
                    sum_r = fmaf(v[r], (float)row, sum_r);
                    sum_c = fmaf(v[r], (float)col, sum_c);
                    sum_p += v[r];
                    if (v[r] > best) { best = v[r]; best_k = k0 + r; }      // ascending keys: strict > keeps the first
                }
                if (++col == p.grid_w) { col = 0; ++row; }
            }
            if (p.map && qok) {
                float* dst = p.map + ((int64_t)b * p.Sq + q) * p.ld_map + k0;
                if (p.map_vec && k0 + 3 < p.Sk) *(float4*)dst = make_float4(v[0], v[1], v[2], v[3]);
                else {
#pragma unroll
                    for (int r = 0; r < 4; ++r) if (k0 + r < p.Sk) dst[r] = v[r];
                }
            }
        }
    }
    // the four lanes of a query hold disjoint keys: two xor steps, the same order on every run
#pragma unroll
    for (int o = 16; o <= 32; o <<= 1) {
        sum_r += __shfl_xor(sum_r, o, 64);
        sum_c += __shfl_xor(sum_c, o, 64);
        sum_p += __shfl_xor(sum_p, o, 64);
        const float ov = __shfl_xor(best, o, 64);
        const int ok = __shfl_xor(best_k, o, 64);
        peak_fold(best, best_k, ov, ok);
    }
    if (qok && g == 0) {
        const int64_t row = (int64_t)b * p.Sq + q;
        if (p.pos) *(float4*)(p.pos + row * 4) = make_float4(sum_r, sum_c, best, sum_p);
        if (p.peak) p.peak[row] = best_k;
    }
}

// ---- per-token scores: one wave per logits row --------------------------------------------------------------------------------------
// Row b * T + t is scored against targets[b][t + 1] (kzv_ce_fwd_bwd's indexing).  ONE pass over the row, 16 bytes per lane: each lane
// keeps the maximum of its columns, its first column and the sum of exp(x - max) under that maximum (rescaled when the maximum moves);
// the lanes are then combined by xor shuffles under the row maximum -- a fixed order (row_scan.h, shared with token_topk.hip).
__global__ __launch_bounds__(256) void token_scores_kernel(const float* __restrict__ logits, int64_t ld, const int64_t* __restrict__ targets,
                                                           int64_t ld_targets, int rows, int T, int vocab, int pad_id, int vec,
                                                           float* __restrict__ logprob, int64_t* __restrict__ top1, float* __restrict__ top1_logprob) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;                                 // wave-uniform; no barrier follows
    const float* lr = logits + (int64_t)row * ld;
    RowScan st;
    const int nv = vec ? vocab >> 2 : 0;                     // float4 pieces (rows 16-byte aligned), then the tail by column
    for (int i = lane; i < nv; i += 64) {
        const float4 x = ((const float4*)lr)[i];
        st.take(x.x, 4 * i); st.take(x.y, 4 * i + 1); st.take(x.z, 4 * i + 2); st.take(x.w, 4 * i + 3);
    }
    for (int j = 4 * nv + lane; j < vocab; j += 64) st.take(lr[j], j);
    float mx = st.mx;
    int arg = st.arg;
    wave_first_argmax(mx, arg);
    const float lse = wave_lse(st, mx);
    if (lane == 0) {
        const int b = row / T, t = row - b * T;
        const int64_t tgt = targets[(int64_t)b * ld_targets + t + 1];
        if (logprob) logprob[row] = (tgt == pad_id || tgt < 0 || tgt >= vocab) ? 0.f : lr[tgt] - lse;
        if (top1) top1[row] = arg == ROW_NO_COL ? 0 : arg;   // (a row without a finite maximum)
        if (top1_logprob) top1_logprob[row] = mx - lse;
    }
}

}  // namespace

extern "C" int kzv_attn_probs(const kzv_attn_probs_args* a, void* stream) {
    if (!a || !a->Q || !a->K || !a->LSE) return kzv_fail(KZV_E_ARG, "attn_probs: null operand");
    if (a->head_dim != 0 && a->head_dim != 64) return kzv_fail(KZV_E_ARG, "attn_probs: head_dim must be 64 (got %d)", a->head_dim);
    if (a->mode != 0) return kzv_fail(KZV_E_ARG, "attn_probs: only mode 0 (no mask; got mode %d)", a->mode);
    if (a->Sq < 1 || a->Sq > KZV_ATTN_MAX_S) return kzv_fail(KZV_E_ARG, "attn_probs: Sq must be in 1..288 (got %d)", a->Sq);
    if (a->Sk < 1 || a->Sk > KZV_ATTN_STREAM_MAX_S) return kzv_fail(KZV_E_ARG, "attn_probs: Sk must be in 1..4097 (got %d)", a->Sk);
    if (a->B < 1 || a->heads < 1 || a->grid_w < 1) return kzv_fail(KZV_E_ARG, "attn_probs: B, heads and grid_w must be positive");
    if ((a->ldq | a->ldk) % 8 || a->ldq < (int64_t)a->heads * 64 || a->ldk < (int64_t)a->heads * 64)
        return kzv_fail(KZV_E_ARG, "attn_probs: row strides must be multiples of 8 and hold heads * 64 columns");
    if (((uintptr_t)a->Q | (uintptr_t)a->K) & 15) return kzv_fail(KZV_E_ARG, "attn_probs: Q and K must be 16-byte aligned");
    if (a->map && a->ld_map < a->Sk) return kzv_fail(KZV_E_ARG, "attn_probs: ld_map %lld < Sk %d", (long long)a->ld_map, a->Sk);
    if (a->pos && ((uintptr_t)a->pos & 15)) return kzv_fail(KZV_E_ARG, "attn_probs: pos must be 16-byte aligned");
    ProbsP p;
    p.Q = (const bf16_t*)a->Q; p.K = (const bf16_t*)a->K; p.LSE = a->LSE; p.map = a->map; p.pos = a->pos; p.peak = a->peak;
    p.ldq = a->ldq; p.ldk = a->ldk; p.ld_map = a->ld_map;
    p.B = a->B; p.heads = a->heads; p.Sq = a->Sq; p.Sk = a->Sk; p.grid_w = a->grid_w; p.nqb = (a->Sq + 63) / 64;
    p.inv_heads = 1.f / (float)a->heads;
    p.map_vec = a->map && a->ld_map % 4 == 0 && ((uintptr_t)a->map & 15) == 0;
    if ((int64_t)a->B * p.nqb >= (1ll << 31)) return kzv_fail(KZV_E_ARG, "attn_probs: grid beyond 2^31 workgroups");
    hipLaunchKernelGGL(attn_probs_kernel, dim3(a->B * p.nqb), dim3(256), 0, (hipStream_t)stream, p);
    return kzv_check_launch("attn_probs");
}

extern "C" int kzv_token_scores(const float* logits, int64_t ld, const int64_t* targets, int64_t ld_targets, int rows_b, int T, int vocab, int pad_id,
                                float* logprob, int64_t* top1, float* top1_logprob, void* stream) {
    if (!logits || !targets) return kzv_fail(KZV_E_ARG, "token_scores: null operand");
    if (rows_b < 1 || T < 1 || vocab < 1 || ld < vocab || ld_targets < (int64_t)T + 1)
        return kzv_fail(KZV_E_ARG, "token_scores: need rows_b, T, vocab >= 1, ld >= vocab and ld_targets >= T + 1");
    const int64_t rows = (int64_t)rows_b * T;
    if (rows >= (1ll << 31)) return kzv_fail(KZV_E_ARG, "token_scores: more than 2^31 rows");
    hipLaunchKernelGGL(token_scores_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, (hipStream_t)stream, logits, ld, targets, ld_targets,
                       (int)rows, T, vocab, pad_id, (ld % 4 == 0 && ((uintptr_t)logits & 15) == 0) ? 1 : 0, logprob, top1, top1_logprob);
    return kzv_check_launch("token_scores");
}
