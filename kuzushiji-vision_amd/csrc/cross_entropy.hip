// Cross-entropy of the decoder's LM head (nn.CrossEntropyLoss(ignore_index = pad), src/models/trocr_model.py:256,292; optional label
// smoothing, class weights and focal term), forward + dlogits, in its three forms: head_ce_kernel (head GEMM and loss in one launch on the row-panel scheme of
// dec_rows.h, logits never written), ce_kernel (materialised logits, the row in registers) and ce_generic_kernel (rows wider than that).
// What the three must agree on -- the smoothed target and the terms it puts into the loss and the gradient -- is CeTarget, and
// CeTargetW under class weights / focal (the W instantiations, whose normaliser {W, S_w} target_weight_sum_kernel sums in a fixed order).
#include "dec_rows.h"
#include "../../include/kzv.h"
#include "kzv_host.h"
#include "kzv_kernels.h"

namespace {

// The target distribution of a row with label y: hot at y plus unif on each of the V real columns -- (1, 0) without label smoothing,
// (1 - eps, eps / V) with it (LS is compile time: the plain instantiations do not read eps) -- and 1 / (number of target tokens).
template <bool LS>
struct CeTarget {
    float inv_cnt, unif, hot;
    __device__ __forceinline__ CeTarget(float eps, int V, const float* count) : inv_cnt(1.f / *count), unif(LS ? eps / (float)V : 0.f), hot(LS ? 1.f - eps : 1.f) {}
    // loss of one row from its log-sum-exp, the target's logit z_y and (LS) the plain sum of its V logits
    __device__ __forceinline__ float loss_row(float lse, float zy, float zsum) const {
        if constexpr (LS) return (lse - hot * zy - unif * zsum) * inv_cnt;
        else return (lse - zy) * inv_cnt;
    }
    // d loss / d z of one REAL column (< V) from its logit z and the row's lse.  The caller guards the padded columns [V, Vp): with
    // smoothing they would hold -unif / count; without it exp(-inf) = 0 covers a caller that fills them with -inf.
    // (ce_kernel holds exp(z - max) in registers and scales by inv_cnt / sum: it rounds differently and keeps its own statement.)
    __device__ __forceinline__ float grad(float z, float lse, bool is_target) const {
        if constexpr (LS) return (__expf(z - lse) - (is_target ? hot : 0.f) - unif) * inv_cnt;
        else return (__expf(z - lse) - (is_target ? 1.f : 0.f)) * inv_cnt;
    }
};

// The sibling of CeTarget for class weights w[V] and the focal exponent gamma (the W instantiations).  The normaliser is
// norm2 = {W, S_w} (target_weight_sum_kernel): W = the sum of w[y] over the scored rows, S_w = the sum of w over the V classes; w == null
// stands for w = 1 (W = the number of scored rows, S_w = V).  A row's gradient is coef softmax - hot onehot - uw w[c], and hot = coef - kd
// with kd the same for every row, so a row carries ONE number into the gradient pass:
//   gamma = 0 (F.cross_entropy(weight = w, label_smoothing = eps)):  coef = ((1 - eps) w_y + (eps / V) S_w) / W,  kd = (eps / V) S_w / W,  uw = eps / (V W)
//   gamma > 0 (focal, eps = 0): with nll = max(lse - z_y, 0), q = 1 - p_y = -expm1(-nll):
//                               coef = w_y (q^gamma + gamma q^(gamma - 1) p_y nll) / W (0 where q = 0),  kd = 0,  uw = 0,  loss = w_y q^gamma nll / W
// Without label smoothing (uw = 0) no class weight but the target's is read.
// The clamp of nll: where the target dominates, fp32 lse - z_y can come out a little below zero, and a negative base under a fractional
// power is NaN.
struct CeTargetW {
    float inv_w, sw, hotk, unif, uw, kd, gamma;
    __device__ __forceinline__ CeTargetW(float eps, int V, const float* norm2, float gamma_)
        : inv_w(1.f / norm2[0]), sw(norm2[1]), hotk(1.f - eps), unif(eps / (float)V), uw(eps / (float)V * (1.f / norm2[0])),
          kd(eps / (float)V * norm2[1] * (1.f / norm2[0])), gamma(gamma_) {}
    // one row from its log-sum-exp, the target's logit z_y and weight w_y, and (eps > 0) sum_c w[c] z_c over its V logits: the coefficient
    // on the softmax and the row's share of the loss
    __device__ __forceinline__ void row(float lse, float zy, float wy, float wzsum, float& coef, float& loss) const {
        if (gamma > 0.f) {
            const float nll = fmaxf(lse - zy, 0.f), q = -expm1f(-nll);
            float f = 0.f, g = 0.f;
            if (q > 0.f) {
                const float q1 = powf(q, gamma - 1.f);
                f = q1 * q;
                g = f + gamma * q1 * (1.f - q) * nll;
            }
            coef = wy * g * inv_w;
            loss = wy * f * nll * inv_w;
        } else {
            coef = hotk * wy * inv_w + kd;
            loss = (hotk * wy * (lse - zy) + unif * (sw * lse - wzsum)) * inv_w;
        }
    }
    // d loss / d z of one REAL column (< V) with class weight wc; the caller guards the padded columns and the ignored rows
    __device__ __forceinline__ float grad(float z, float lse, bool is_target, float coef, float wc) const {
        return coef * __expf(z - lse) - (is_target ? coef - kd : 0.f) - uw * wc;
    }
};
// w[c] of a real column, 0 beyond the vocabulary (nothing is read there); w == null: every class weighs 1
__device__ __forceinline__ float class_weight(const float* w, int c, int V) { return c < V ? (w ? w[c] : 1.f) : 0.f; }
// a label the loss scores: not pad and inside the vocabulary (the weight of anything else is never read)
__device__ __forceinline__ bool scored_label(int64_t g, int pad, int V) { return g != pad && g >= 0 && g < V; }

// ---- the normaliser of the weighted loss: out[0] = W = sum of w[labels[b][t + 1]] over the scored rows, out[1] = S_w = sum_{c < V} w[c] ----
// One workgroup, every partial sum in a fixed order (lane-strided sums, the wave's butterfly, the 16 waves in turn): every gradient of the
// step is scaled by 1 / W, which must not move in the last place from run to run the way an atomic sum does.  w == null: W = the count, S_w = V.
__global__ __launch_bounds__(1024) void target_weight_sum_kernel(const int64_t* __restrict__ labels, int L, int B, int T, int V, int pad,
                                                                 const float* __restrict__ w, float* __restrict__ out) {
    __shared__ float red[2][16];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    float a = 0.f, b = 0.f;
    for (int i = tid; i < B * T; i += 1024) {
        const int bb = i / T, t = i - bb * T;
        const int64_t g = labels[(int64_t)bb * L + t + 1];
        if (scored_label(g, pad, V)) a += w ? w[g] : 1.f;
    }
    for (int c = tid; c < V; c += 1024) b += w ? w[c] : 1.f;
    a = wave_sum(a); b = wave_sum(b);
    if (lane == 0) { red[0][wv] = a; red[1][wv] = b; }
    __syncthreads();
    if (tid == 0) {
        float sa = 0.f, sb = 0.f;
        for (int k = 0; k < 16; ++k) { sa += red[0][k]; sb += red[1][k]; }
        out[0] = sa; out[1] = sb;
    }
}

// ---- LM head + cross-entropy in one launch, logits never materialised (round 4, VERDICT r03 "missing" 1) -------------
// Replaces, for a training / validation step that does not return logits: lm_head.decoder (HF modeling_roberta.py:888-893, tied to the
// word embeddings) + CrossEntropyLoss(ignore_index = pad) (src/models/trocr_model.py:256,292) -- a [B*T, 4352] fp32 logits tensor written
// by the GEMM (267 MB at T = 60), read back by ce_kernel, and the bf16 gradient written behind it.  Rows are independent: one workgroup
// takes 64 rows of the head's LayerNorm output (bf16, in LDS) against the whole vocabulary twice, 256 columns at a time, the tied
// weight arriving in fragment order from L2 (2.2 MB, shared by every workgroup) through chain_gemm's window:
//   pass 1: logits chunk -> per-lane online (max, sum exp) over the lane's own columns, the target's logit picked out on the way;
//           the 32 partial pairs of a row (8 waves x 4 lane groups) meet in LDS -> lse[row]; loss += (lse - logit[target]) / count
//   pass 2: the same chunks again -> (exp(logit - lse) - onehot) / count as bf16 through an LDS tile, whole rows out (dlogits, the
//           operand of the head's two gradient GEMMs).  Skipped without a gradient buffer (validation).
// Same arithmetic as gemm_nt + ce_kernel up to fp32 summation order (bf16 operands, fp32 accumulation, fp32 softmax statistics).
// LS (compile time; label smoothing, F.cross_entropy(label_smoothing = eps), eps in (0, 1)): the target distribution is (1 - eps) onehot +
// eps / V over the V real columns.  Pass 1 keeps a third running statistic per lane, the plain sum of its logits in columns < V (the -inf
// fill of the padded columns stays out of it); the 32 partial sums of a row meet in LDS behind the other row arrays and are folded in the
// same fixed order: loss_row = lse - (1 - eps) logit[target] - (eps / V) sum.  Pass 2 writes (exp(logit - lse) - (1 - eps) onehot - eps / V)
// / count in columns < V and ZERO in columns [V, Vp) by an explicit guard: without smoothing exp(-inf) = 0 covers them, with it they
// would hold -eps / (V count) and enter the head's two gradient GEMMs and the fused dh.  LS = false is the kernel as it was.
// W (compile time; class weights and / or the focal exponent, CeTargetW; LS is then false and eps a run-time value): p.count holds
// {W, S_w}.  The row's one thread derives the row's coefficient on the softmax in the fold and leaves it in coef_s for pass 2; its loss
// share goes into the wave sum.  Under smoothing (a wave-uniform test of eps) pass 1's third statistic is sum_c w[c] z_c and pass 2
// subtracts uw w[c], the weights read the way the bias is; without it no class weight but the target's is read.  The padded columns and the
// ignored rows are zeroed by the LS form's guard.  W = false is the kernel as it was.
struct HeadCE {
    const bf16_t* x; const bf16_t* wp; const float* bias; const int64_t* labels; const float* count; float* loss; bf16_t* dlogits;
    int M, L, T, V, Vp, nch, pad;
    const bf16_t* wpt; bf16_t* dh;      // optional: dh[M, 256] = dlogits . W (the head's input gradient), wpt = W^T [256, 256 nch] in fragment order
    float eps;                          // label smoothing (read by the LS and W instantiations only)
    const float* cw; float gamma;       // W instantiations only: class weights [V] or null (w = 1), the focal exponent; count is then {W, S_w}
};
constexpr int LDS_HEAD = 2 * LDS_A1 + RM * 64 * 4 + RM * 4 * 3;           // head_ce_kernel<*, false>
constexpr int LDS_HEAD_LS = LDS_HEAD + RM * 32 * 4;                        // + the 32 partial logit sums of every row
constexpr int LDS_HEAD_W = LDS_HEAD_LS + RM * 4;                           // + every row's coefficient on the softmax
static_assert(LDS_HEAD == 84736 && LDS_HEAD_LS == 92928 && LDS_HEAD_W == 93184, "head_ce: dynamic LDS");
template <bool DH, bool LS, bool W>
__global__ __launch_bounds__(512) void head_ce_kernel(const HeadCE p) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    bf16_t* a1 = (bf16_t*)smem;                                   // [RM][LDH] the rows' operand tile
    bf16_t* stage = (bf16_t*)(smem + LDS_A1);                     // [RM][LDH] one chunk of dlogits on its way out
    float* red = (float*)(smem + 2 * LDS_A1);                     // [RM][32][2] partial (max, sum) pairs
    float* lse_s = red + RM * 64;                                 // [RM]
    float* tl_s = lse_s + RM;                                     // [RM] the target's logit
    int* tgt_s = (int*)(tl_s + RM);                               // [RM] target class, -1 = ignored row
    float* zsum = (float*)(tgt_s + RM);                           // LS only: [RM][32] partial plain sums of the row's logits (W: of w[c] z_c)
    float* coef_s = zsum + RM * 32;                               // W only: [RM] the row's coefficient on the softmax
    const int tid = threadIdx.x, lane0 = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int m0 = blockIdx.x * RM;
    bf16x8 R[WIN];
    fill_window<2, 8, NW, WIN>(R, wave_frags<2, 8>(p.wp, w), opaque(lane0));
    load_rows(p.x, a1, m0, p.M, opaque(tid));
    if (tid < RM) {
        const int m = m0 + tid;
        int t = -1;
        if (m < p.M) {
            const int b = m / p.T, pos = m - b * p.T;
            const int64_t g = p.labels[(int64_t)b * p.L + pos + 1];
            t = (g == p.pad || g < 0 || g >= p.V) ? -1 : (int)g;
        }
        tgt_s[tid] = t; tl_s[tid] = 0.f;
    }
    wg_barrier();
    const int lane = opaque(lane0), l15 = lane & 15, g = lane >> 4;
    int tg[RT];
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) tg[rt] = tgt_s[rt * 16 + l15];
    const CeTarget<LS> ce(p.eps, p.V, p.count);
    // the chunk's logits of this lane: v[c][rt][r] at column n0(c) + r, row rt * 16 + l15; columns >= V -> -inf
    auto chunk_logits = [&](int j, const f32x4 (&acc)[2][RT], float (&v)[2][RT][4]) {
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            const int n0 = j * 256 + (w + 8 * c) * 16 + 4 * g;
            float bb[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) bb[r] = n0 + r < p.V ? p.bias[n0 + r] : 0.f;
#pragma unroll
            for (int rt = 0; rt < RT; ++rt)
#pragma unroll
                for (int r = 0; r < 4; ++r) v[c][rt][r] = n0 + r < p.V ? acc[c][rt][r] + bb[r] : -INFINITY;
        }
    };
    const bool smooth = W && p.eps > 0.f;             // W: the per-column weights enter only under label smoothing (wave-uniform)
    // ---- pass 1 ----
    float mrun[RT], lrun[RT], zrun[RT];
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) { mrun[rt] = -INFINITY; lrun[rt] = 0.f; zrun[rt] = 0.f; }
#pragma unroll 1
    for (int j = 0; j < p.nch; ++j) {
        f32x4 acc[2][RT];
        const bf16_t* nextw = p.wp + (int64_t)(j + 1 < p.nch ? j + 1 : 0) * 65536;          // the last chunk prefetches pass 2's first
        chain_gemm<2, 8, 2, 8, true>(R, wave_frags<2, 8>(p.wp + (int64_t)j * 65536, w), wave_frags<2, 8>(nextw, w), a1, LDH, lane, acc);
        float v[2][RT][4];
        chunk_logits(j, acc, v);
        float wz[2][4];                                                       // W only: the class weights of the lane's eight columns, read the way the bias is
        if constexpr (W) {
#pragma unroll
            for (int c = 0; c < 2; ++c)
#pragma unroll
                for (int r = 0; r < 4; ++r) wz[c][r] = smooth ? class_weight(p.cw, j * 256 + (w + 8 * c) * 16 + 4 * g + r, p.V) : 0.f;
        }
#pragma unroll
        for (int rt = 0; rt < RT; ++rt) {
            float mx = mrun[rt];
#pragma unroll
            for (int c = 0; c < 2; ++c)
#pragma unroll
                for (int r = 0; r < 4; ++r) mx = fmaxf(mx, v[c][rt][r]);
            if (mx > -INFINITY) {
                float sacc = lrun[rt] * __expf(mrun[rt] - mx);            // (exp(-inf - finite) = 0 on the first finite chunk)
#pragma unroll
                for (int c = 0; c < 2; ++c)
#pragma unroll
                    for (int r = 0; r < 4; ++r) sacc += __expf(v[c][rt][r] - mx);
                lrun[rt] = sacc; mrun[rt] = mx;
            }
            if constexpr (LS) {                                               // plain sum over the columns the vocabulary has (-inf marks the others)
#pragma unroll
                for (int c = 0; c < 2; ++c)
#pragma unroll
                    for (int r = 0; r < 4; ++r) zrun[rt] += v[c][rt][r] == -INFINITY ? 0.f : v[c][rt][r];
            }
            if constexpr (W) {                                                // the same sum under the class weights; only smoothing needs it
#pragma unroll
                for (int c = 0; c < 2; ++c)
#pragma unroll
                    for (int r = 0; r < 4; ++r) zrun[rt] += wz[c][r] != 0.f ? wz[c][r] * v[c][rt][r] : 0.f;      // (0: beyond V, where v is -inf)
            }
#pragma unroll
            for (int c = 0; c < 2; ++c) {
                const int n0 = j * 256 + (w + 8 * c) * 16 + 4 * g;
                const int d = tg[rt] - n0;
                if (d >= 0 && d < 4) tl_s[rt * 16 + l15] = d == 0 ? v[c][rt][0] : d == 1 ? v[c][rt][1] : d == 2 ? v[c][rt][2] : v[c][rt][3];
            }
        }
    }
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) {
        float* q = red + ((rt * 16 + l15) * 32 + w * 4 + g) * 2;
        q[0] = mrun[rt]; q[1] = lrun[rt];
        if constexpr (LS || W) zsum[(rt * 16 + l15) * 32 + w * 4 + g] = zrun[rt];
    }
    wg_barrier();
    if (tid < RM) {                                   // one thread per row folds the 32 pairs in a fixed order
        float mx = -INFINITY;
        for (int k = 0; k < 32; ++k) mx = fmaxf(mx, red[(tid * 32 + k) * 2]);
        float se = 0.f;
        for (int k = 0; k < 32; ++k) se += red[(tid * 32 + k) * 2 + 1] * __expf(red[(tid * 32 + k) * 2] - mx);
        const float lse = mx + __logf(se);
        lse_s[tid] = lse;
        float zs = 0.f;
        if constexpr (LS || W) {
            for (int k = 0; k < 32; ++k) zs += zsum[tid * 32 + k];
        }
        float contrib = 0.f;
        if constexpr (W) {                            // the row's coefficient and loss share, once per row; pass 2 reads the coefficient back
            float coef = 0.f;
            if (tgt_s[tid] >= 0) CeTargetW(p.eps, p.V, p.count, p.gamma).row(lse, tl_s[tid], class_weight(p.cw, tgt_s[tid], p.V), zs, coef, contrib);
            coef_s[tid] = coef;
        } else {
            contrib = tgt_s[tid] >= 0 ? ce.loss_row(lse, tl_s[tid], zs) : 0.f;
        }
        contrib = wave_sum(contrib);
        if (tid == 0) atomicAdd(p.loss, contrib);
    }
    if (!p.dlogits) return;                           // wave-uniform (a kernel argument)
    wg_barrier();
    float ls[RT];
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) ls[rt] = lse_s[rt * 16 + l15];
    float cf[RT];                                     // W only: the rows' coefficients on the softmax
    const CeTargetW cwt(W ? p.eps : 0.f, p.V, p.count, W ? p.gamma : 0.f);
    if constexpr (W) {
#pragma unroll
        for (int rt = 0; rt < RT; ++rt) cf[rt] = coef_s[rt * 16 + l15];
    }
    // ---- pass 2 ----
    // With wpt / dh the head's input gradient rides along: dh = dlogits . W accumulates chunk by chunk from the staged dlogits tile (the
    // launch it replaces read the 134 MB of dlogits back: 92 us in the step), the window alternating between the two weight streams.
    constexpr bool with_dh = DH;                                               // compile time: no run-time branch around a load (see pin)
    const int KSV = p.nch * 8;                                                 // 32-deep steps of the vocabulary in the transposed pack
    const unsigned wo = (unsigned)lane * 16u;
    auto tfrag = [&](int j, int i) -> bf16x8 {                                 // fragment i = (vocabulary step 8 j + i / 2, hidden column block w + 8 (i % 2))
        return *(const bf16x8*)((const char*)p.wpt + ((int64_t)(w + 8 * (i & 1)) * KSV + 8 * j + (i >> 1)) * 1024 + wo);
    };
    f32x4 acc2[2][RT];
#pragma unroll
    for (int c = 0; c < 2; ++c)
#pragma unroll
        for (int rt = 0; rt < RT; ++rt) acc2[c][rt] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll 1
    for (int j = 0; j < p.nch; ++j) {
        f32x4 acc[2][RT];
        if constexpr (with_dh) {
            chain_gemm<2, 8, 2, 8, false>(R, wave_frags<2, 8>(p.wp + (int64_t)j * 65536, w), nullptr, a1, LDH, lane, acc);
#pragma unroll
            for (int i = 0; i < WIN; ++i) R[i] = tfrag(j, i);                  // in flight under the softmax arithmetic below
        } else {
            if (j + 1 < p.nch) chain_gemm<2, 8, 2, 8, true>(R, wave_frags<2, 8>(p.wp + (int64_t)j * 65536, w), wave_frags<2, 8>(p.wp + (int64_t)(j + 1) * 65536, w), a1, LDH, lane, acc);
            else chain_gemm<2, 8, 2, 8, false>(R, wave_frags<2, 8>(p.wp + (int64_t)j * 65536, w), nullptr, a1, LDH, lane, acc);
        }
        float v[2][RT][4];
        chunk_logits(j, acc, v);
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            const int nl = (w + 8 * c) * 16 + 4 * g, n0 = j * 256 + nl;
            float wc[4];                                                       // W only: the class weights of the lane's four columns
            if constexpr (W) {
#pragma unroll
                for (int r = 0; r < 4; ++r) wc[r] = smooth ? class_weight(p.cw, n0 + r, p.V) : 0.f;
            }
#pragma unroll
            for (int rt = 0; rt < RT; ++rt) {
                float o[4];
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    if constexpr (W) o[r] = tg[rt] >= 0 && n0 + r < p.V ? cwt.grad(v[c][rt][r], ls[rt], n0 + r == tg[rt], cf[rt], wc[r]) : 0.f;      // the guard, as under LS
                    else if constexpr (LS) o[r] = tg[rt] >= 0 && n0 + r < p.V ? ce.grad(v[c][rt][r], ls[rt], n0 + r == tg[rt]) : 0.f;      // padded columns: the guard
                    else o[r] = tg[rt] >= 0 ? (__expf(v[c][rt][r] - ls[rt]) - (n0 + r == tg[rt] ? 1.f : 0.f)) * ce.inv_cnt : 0.f;      // exp(-inf) = 0: padded columns
                }
                *(uint2*)(stage + (rt * 16 + l15) * LDH + nl) = make_uint2(pack_bf2(o[0], o[1]), pack_bf2(o[2], o[3]));
            }
        }
        wg_barrier();
        {                                             // whole rows out: 16 bytes per lane, only the columns dlogits has (Vp may end inside the chunk).
                                                      // (rows_out's loop with a piece count; its own spelling -- shifts -- so it stays here: DESIGN 4l)
            const int pieces = min(32, (p.Vp - j * 256) / 8);
            const int t2 = opaque(tid);
#pragma unroll
            for (int q = 0; q < RM * 32 / 512; ++q) {
                const int idx = t2 + q * 512, row = idx >> 5, ch = idx & 31;
                if (m0 + row < p.M && ch < pieces) *(uint4*)(p.dlogits + (int64_t)(m0 + row) * p.Vp + j * 256 + ch * 8) = *(const uint4*)(stage + row * LDH + ch * 8);
            }
        }
        if constexpr (with_dh) {                          // acc2 += (this chunk of dlogits) . W^T fragments; then the window goes back to the forward stream
            const bf16_t* ap = stage + l15 * LDH + g * 8;
            bf16x8 fa[RT];
#pragma unroll
            for (int i = 0; i < WIN; ++i) {
                if ((i & 1) == 0) {
#pragma unroll
                    for (int rt = 0; rt < RT; ++rt) fa[rt] = *(const bf16x8*)(ap + rt * 16 * LDH + (i >> 1) * 32);
                }
#pragma unroll
                for (int rt = 0; rt < RT; ++rt) acc2[i & 1][rt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(R[i], fa[rt], acc2[i & 1][rt], 0, 0, 0);
            }
            const int jn = j + 1 < p.nch ? j + 1 : 0;     // (the last refill is unused: no branch around the loads)
#pragma unroll
            for (int i = 0; i < WIN; ++i) R[i] = ld_frag<2, 8, NW>(wave_frags<2, 8>(p.wp + (int64_t)jn * 65536, w), wo, i);
        }
        wg_barrier();
    }
    if constexpr (with_dh) {                              // dh rows out through the stage tile (bf16, as the GEMM epilogue rounded them)
        // (bf16_to_lds without a bias, spelled here: through the helper the eight stores pair up differently and the code object moves)
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            const int nl = (w + 8 * c) * 16 + 4 * g;
#pragma unroll
            for (int rt = 0; rt < RT; ++rt)
                *(uint2*)(stage + (rt * 16 + l15) * LDH + nl) = make_uint2(pack_bf2(acc2[c][rt][0], acc2[c][rt][1]), pack_bf2(acc2[c][rt][2], acc2[c][rt][3]));
        }
        wg_barrier();
        rows_out<32>(stage, LDH, p.dh, HD, m0, p.M, opaque(tid));
    }
}

// ---- cross-entropy of materialised logits (a step that returns them, or KZV_HEAD_CE = 0) ------------------------------------------------
// one workgroup per token row; target = labels[b][t+1]; rows whose target is pad contribute nothing and
// get a zero dlogits row.  dlogits = (softmax - onehot) / count, bf16, pad columns [V, ldl) zeroed.
// LS (compile time; label smoothing eps in (0, 1), F.cross_entropy(label_smoothing = eps)): the target distribution is (1 - eps) onehot +
// eps / V over the V real columns, so loss_row = lse - (1 - eps) z[y] - (eps / V) sum_{v < V} z[v] and dlogits = (softmax - (1 - eps) onehot
// - eps / V) / count in columns < V; columns [V, ldl) stay zero by an explicit guard (exp(-inf) = 0 no longer covers them).  One more block
// reduction (the plain logit sum).  LS = false is the kernel as it was: eps is not read.
__device__ __forceinline__ float finite_or_zero(float x) { return x == -INFINITY ? 0.f : x; }
template <bool LS, bool W>
__global__ __launch_bounds__(256) void ce_kernel(const float* __restrict__ logits, int64_t ldl, const int64_t* __restrict__ labels,
                                                 int L, int T, int V, int pad, const float* __restrict__ count,
                                                 float* loss, bf16_t* __restrict__ dlogits, float eps, const float* __restrict__ cw, float gamma) {
    __shared__ float red[LS || W ? 12 : 8];
    const int row = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int b = row / T, t = row - b * T;
    const int64_t tgt = labels[(int64_t)b * L + t + 1];
    const float* lr = logits + (int64_t)row * ldl;
    bf16_t* dr = dlogits ? dlogits + (int64_t)row * ldl : nullptr;
    const int n4 = (int)(ldl / 4);
    if (W ? !scored_label(tgt, pad, V) : tgt == pad) {      // (W: a label outside the vocabulary has no weight to read and is not scored either)
        if (dr) for (int i = tid; i < n4; i += 256) ((uint2*)dr)[i] = make_uint2(0, 0);
        return;
    }
    // the row lives in registers (ldl / 4 <= 256 * RV float4 pieces): read once, 16 bytes per lane
    constexpr int RV = 5;                                  // 5 * 256 * 4 = 5120 columns
    float4 v[RV];
    float mx = -INFINITY;
#pragma unroll
    for (int j = 0; j < RV; ++j) {
        const int i = tid + j * 256;
        v[j] = make_float4(-INFINITY, -INFINITY, -INFINITY, -INFINITY);
        if (i < n4) {
            v[j] = ((const float4*)lr)[i];
            if (4 * i + 1 > V) v[j].x = -INFINITY;      // pad columns [V, ldl) hold zeros, not logits
            if (4 * i + 2 > V) v[j].y = -INFINITY;
            if (4 * i + 3 > V) v[j].z = -INFINITY;
            if (4 * i + 4 > V) v[j].w = -INFINITY;
        }
        mx = fmaxf(fmaxf(mx, fmaxf(v[j].x, v[j].y)), fmaxf(v[j].z, v[j].w));
    }
    float sz = 0.f;                                         // LS: the plain sum of the row's V logits, taken before the registers turn into exponentials
    if constexpr (LS) {
#pragma unroll
        for (int j = 0; j < RV; ++j) sz += (finite_or_zero(v[j].x) + finite_or_zero(v[j].y)) + (finite_or_zero(v[j].z) + finite_or_zero(v[j].w));
        sz = wave_sum(sz);
        if (lane == 0) red[8 + w] = sz;
    }
    if constexpr (W) {                                      // W: the sum of w[c] z_c instead (class_weight is 0 in the columns that hold -inf)
#pragma unroll
        for (int j = 0; j < RV; ++j) {
            const int c0 = 4 * (tid + j * 256);
            sz += (class_weight(cw, c0, V) * finite_or_zero(v[j].x) + class_weight(cw, c0 + 1, V) * finite_or_zero(v[j].y))
                + (class_weight(cw, c0 + 2, V) * finite_or_zero(v[j].z) + class_weight(cw, c0 + 3, V) * finite_or_zero(v[j].w));
        }
        sz = wave_sum(sz);
        if (lane == 0) red[8 + w] = sz;
    }
    mx = wave_max(mx);
    if (lane == 0) red[w] = mx;
    __syncthreads();
    mx = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
    if constexpr (LS || W) sz = (red[8] + red[9]) + (red[10] + red[11]);
    float se = 0.f;
#pragma unroll
    for (int j = 0; j < RV; ++j) {
        v[j].x = __expf(v[j].x - mx); v[j].y = __expf(v[j].y - mx); v[j].z = __expf(v[j].z - mx); v[j].w = __expf(v[j].w - mx);
        se += (v[j].x + v[j].y) + (v[j].z + v[j].w);
    }
    se = wave_sum(se);
    if (lane == 0) red[4 + w] = se;
    __syncthreads();
    se = red[4] + red[5] + red[6] + red[7];
    const float lse = mx + __logf(se);
    if constexpr (W) {                                      // every thread derives the row's terms (a few dozen flops) instead of a broadcast
        const CeTargetW ct(eps, V, count, gamma);
        float coef, share;
        ct.row(lse, lr[tgt], class_weight(cw, (int)tgt, V), sz, coef, share);
        if (tid == 0) atomicAdd(loss, share);
        if (dr) {
            const float sc = coef / se;                     // coef softmax = coef exp(x - mx) / se, as below
#pragma unroll
            for (int j = 0; j < RV; ++j) {
                const int i = tid + j * 256;
                if (i < n4) {
                    float o[4] = {v[j].x * sc, v[j].y * sc, v[j].z * sc, v[j].w * sc};
                    const int64_t d = tgt - 4 * (int64_t)i;
#pragma unroll
                    for (int r = 0; r < 4; ++r) o[r] = 4 * i + r < V ? o[r] - (d == r ? coef - ct.kd : 0.f) - (eps > 0.f ? ct.uw * class_weight(cw, 4 * i + r, V) : 0.f) : 0.f;
                    ((uint2*)dr)[i] = make_uint2(pack_bf2(o[0], o[1]), pack_bf2(o[2], o[3]));
                }
            }
        }
        return;
    }
    const CeTarget<LS> ce(eps, V, count);
    if (tid == 0) atomicAdd(loss, ce.loss_row(lse, lr[tgt], sz));
    if (dr) {
        // the gradient from the exponentials in registers: scaled by inv_cnt / se first, the target terms subtracted afterwards -- another
        // rounding than CeTarget::grad, so this kernel keeps its own statement
        const float inv_cnt = ce.inv_cnt, hot = ce.hot, unif = ce.unif;
        const float sc = inv_cnt / se;                     // softmax = exp(x - mx) / se
#pragma unroll
        for (int j = 0; j < RV; ++j) {
            const int i = tid + j * 256;
            if (i < n4) {
                float o[4] = {v[j].x * sc, v[j].y * sc, v[j].z * sc, v[j].w * sc};
                const int64_t d = tgt - 4 * (int64_t)i;
                if constexpr (LS) {
#pragma unroll
                    for (int r = 0; r < 4; ++r) o[r] = 4 * i + r < V ? o[r] - (d == r ? hot : 0.f) * inv_cnt - unif * inv_cnt : 0.f;
                } else {
                    if (d >= 0 && d < 4) o[d] -= inv_cnt;
                }
                ((uint2*)dr)[i] = make_uint2(pack_bf2(o[0], o[1]), pack_bf2(o[2], o[3]));
            }
        }
    }
}

// the same for rows wider than the registers of ce_kernel hold (> 5120 columns): three passes over the (L2-resident) row
// one workgroup per token row; target = labels[b][t+1]; rows whose target is pad contribute nothing and
// get a zero dlogits row.  dlogits = (softmax - onehot) / count, bf16, pad columns [V, ldl) zeroed.
// LS: ce_kernel's label smoothing, the logit sum riding in the first pass.
template <bool LS, bool W>
__global__ __launch_bounds__(256) void ce_generic_kernel(const float* __restrict__ logits, int64_t ldl, const int64_t* __restrict__ labels,
                                                 int L, int T, int V, int pad, const float* __restrict__ count,
                                                 float* loss, bf16_t* __restrict__ dlogits, float eps, const float* __restrict__ cw, float gamma) {
    __shared__ float red[LS || W ? 12 : 8];
    const int row = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int b = row / T, t = row - b * T;
    const int64_t tgt = labels[(int64_t)b * L + t + 1];
    const float* lr = logits + (int64_t)row * ldl;
    bf16_t* dr = dlogits ? dlogits + (int64_t)row * ldl : nullptr;
    const int n4 = (int)(ldl / 4);
    if (W ? !scored_label(tgt, pad, V) : tgt == pad) {      // (W: a label outside the vocabulary has no weight to read and is not scored either)
        if (dr) for (int i = tid; i < n4; i += 256) ((uint2*)dr)[i] = make_uint2(0, 0);
        return;
    }
    float mx = -INFINITY, sz = 0.f;
    if constexpr (W) {
        for (int i = tid; i < V; i += 256) { const float z = lr[i]; mx = fmaxf(mx, z); sz += class_weight(cw, i, V) * z; }
        sz = wave_sum(sz);
        if (lane == 0) red[8 + w] = sz;
    } else if constexpr (LS) {
        for (int i = tid; i < V; i += 256) { const float z = lr[i]; mx = fmaxf(mx, z); sz += z; }
        sz = wave_sum(sz);
        if (lane == 0) red[8 + w] = sz;
    } else {
        for (int i = tid; i < V; i += 256) mx = fmaxf(mx, lr[i]);
    }
    mx = wave_max(mx);
    if (lane == 0) red[w] = mx;
    __syncthreads();
    mx = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
    if constexpr (LS || W) sz = (red[8] + red[9]) + (red[10] + red[11]);
    float se = 0.f;
    for (int i = tid; i < V; i += 256) se += __expf(lr[i] - mx);
    se = wave_sum(se);
    if (lane == 0) red[4 + w] = se;
    __syncthreads();
    se = red[4] + red[5] + red[6] + red[7];
    const float lse = mx + __logf(se);
    if constexpr (W) {
        const CeTargetW ct(eps, V, count, gamma);
        float coef, share;
        ct.row(lse, lr[tgt], class_weight(cw, (int)tgt, V), sz, coef, share);
        if (tid == 0) atomicAdd(loss, share);
        if (dr) {
            for (int i = tid; i < n4; i += 256) {
                float v[4];
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int col = 4 * i + r;
                    v[r] = col < V ? ct.grad(lr[col], lse, col == tgt, coef, eps > 0.f ? class_weight(cw, col, V) : 0.f) : 0.f;
                }
                ((uint2*)dr)[i] = make_uint2(pack_bf2(v[0], v[1]), pack_bf2(v[2], v[3]));
            }
        }
        return;
    }
    const CeTarget<LS> ce(eps, V, count);
    if (tid == 0) atomicAdd(loss, ce.loss_row(lse, lr[tgt], sz));
    if (dr) {
        for (int i = tid; i < n4; i += 256) {
            float v[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int col = 4 * i + r;
                v[r] = col < V ? ce.grad(lr[col], lse, col == tgt) : 0.f;
            }
            ((uint2*)dr)[i] = make_uint2(pack_bf2(v[0], v[1]), pack_bf2(v[2], v[3]));
        }
    }
}

}  // namespace

int kzv_head_ce(const KzvHeadCE& a, hipStream_t s) {
    if (!a.x || !a.wp || !a.bias || !a.labels || !a.count || !a.loss || a.M < 1 || a.V < 1 || a.Vp % 8 || a.Vp < a.V) return kzv_fail(KZV_E_ARG, "head_ce: bad argument");
    HeadCE p;
    p.x = a.x; p.wp = a.wp; p.bias = a.bias; p.labels = a.labels; p.count = a.count; p.loss = a.loss; p.dlogits = a.dlogits;
    p.M = a.M; p.L = a.L; p.T = a.T; p.V = a.V; p.Vp = a.Vp; p.nch = (a.V + 255) / 256; p.pad = a.pad;
    p.wpt = (a.dlogits && a.dh) ? a.wpt : nullptr; p.dh = a.dh;
    if (!(a.label_smoothing >= 0.f && a.label_smoothing < 1.f)) return kzv_fail(KZV_E_ARG, "head_ce: label_smoothing %g is not in [0, 1)", (double)a.label_smoothing);
    p.eps = a.label_smoothing;
    if (!kzv_focal_ok(a.focal_gamma, a.label_smoothing)) return kzv_fail(KZV_E_ARG, "head_ce: focal_gamma %g is not in [0, 5], or meets label smoothing", (double)a.focal_gamma);
    p.cw = a.class_weights; p.gamma = a.focal_gamma;
    const dim3 grid((a.M + RM - 1) / RM), block(512);
    if (p.cw || p.gamma > 0.f) {                      // class weights or focal: the W instantiations, a.count = {W, S_w} (kzv_target_weight_sum)
        if (p.wpt) kzv_launch_lds<head_ce_kernel<true, false, true>>(grid, block, LDS_HEAD_W, s, p);
        else kzv_launch_lds<head_ce_kernel<false, false, true>>(grid, block, LDS_HEAD_W, s, p);
    } else if (p.eps > 0.f) {                                // eps = 0: the plain instantiations, the kernel as it was before label smoothing
        if (p.wpt) kzv_launch_lds<head_ce_kernel<true, true, false>>(grid, block, LDS_HEAD_LS, s, p);
        else kzv_launch_lds<head_ce_kernel<false, true, false>>(grid, block, LDS_HEAD_LS, s, p);
    } else {
        if (p.wpt) kzv_launch_lds<head_ce_kernel<true, false, false>>(grid, block, LDS_HEAD, s, p);
        else kzv_launch_lds<head_ce_kernel<false, false, false>>(grid, block, LDS_HEAD, s, p);
    }
    return kzv_check_launch("head_ce");
}

int kzv_ce_fwd_bwd(const float* logits, int64_t ldl, const int64_t* labels, int L, int B, int T, int V, int pad,
                   const float* count, float* loss, bf16_t* dlogits, float label_smoothing, hipStream_t s, const float* class_weights, float focal_gamma) {
    if (ldl % 4) return kzv_fail(KZV_E_ARG, "ce: ldl %% 4");
    if (!(label_smoothing >= 0.f && label_smoothing < 1.f)) return kzv_fail(KZV_E_ARG, "ce: label_smoothing %g is not in [0, 1)", (double)label_smoothing);
    if (!kzv_focal_ok(focal_gamma, label_smoothing)) return kzv_fail(KZV_E_ARG, "ce: focal_gamma %g is not in [0, 5], or meets label smoothing", (double)focal_gamma);
    const float eps = label_smoothing;
    if (class_weights || focal_gamma > 0.f) {         // the W instantiations: count = {W, S_w} (kzv_target_weight_sum)
        if (ldl <= 5120) hipLaunchKernelGGL((ce_kernel<false, true>), dim3(B * T), dim3(256), 0, s, logits, ldl, labels, L, T, V, pad, count, loss, dlogits, eps, class_weights, focal_gamma);
        else hipLaunchKernelGGL((ce_generic_kernel<false, true>), dim3(B * T), dim3(256), 0, s, logits, ldl, labels, L, T, V, pad, count, loss, dlogits, eps, class_weights, focal_gamma);
        return kzv_check_launch("ce_fwd_bwd");
    }
    // eps = 0 launches the plain kernels (the LS = false instantiations: the kernels as they were before label smoothing)
    if (ldl <= 5120) {
        if (eps > 0.f) hipLaunchKernelGGL((ce_kernel<true, false>), dim3(B * T), dim3(256), 0, s, logits, ldl, labels, L, T, V, pad, count, loss, dlogits, eps, (const float*)nullptr, 0.f);
        else hipLaunchKernelGGL((ce_kernel<false, false>), dim3(B * T), dim3(256), 0, s, logits, ldl, labels, L, T, V, pad, count, loss, dlogits, 0.f, (const float*)nullptr, 0.f);
    } else {
        if (eps > 0.f) hipLaunchKernelGGL((ce_generic_kernel<true, false>), dim3(B * T), dim3(256), 0, s, logits, ldl, labels, L, T, V, pad, count, loss, dlogits, eps, (const float*)nullptr, 0.f);
        else hipLaunchKernelGGL((ce_generic_kernel<false, false>), dim3(B * T), dim3(256), 0, s, logits, ldl, labels, L, T, V, pad, count, loss, dlogits, 0.f, (const float*)nullptr, 0.f);
    }
    return kzv_check_launch("ce_fwd_bwd");
}

// per-op C ABI (include/kzv.h, unit parity tests): both forward to the launcher above, which does the validation
extern "C" int kzv_ce_fwd_bwd(const float* logits, int64_t ldl, const int64_t* labels, int L, int B, int T, int V, int pad,
                              const float* count, float* loss, void* dlogits_bf16, void* stream) {
    return kzv_ce_fwd_bwd(logits, ldl, labels, L, B, T, V, pad, count, loss, (bf16_t*)dlogits_bf16, 0.f, (hipStream_t)stream);
}

extern "C" int kzv_ce_fwd_bwd_ls(const float* logits, int64_t ldl, const int64_t* labels, int L, int B, int T, int V, int pad,
                                 const float* count, float* loss, void* dlogits_bf16, float label_smoothing, void* stream) {
    return kzv_ce_fwd_bwd(logits, ldl, labels, L, B, T, V, pad, count, loss, (bf16_t*)dlogits_bf16, label_smoothing, (hipStream_t)stream);
}

// the normaliser {W, S_w} of the weighted loss; d_class_weights == NULL: {the number of scored rows, V}
int kzv_target_weight_sum(const int64_t* labels, int L, int B, int T, int V, int pad, const float* d_class_weights, float* d_out2, hipStream_t s) {
    if (!labels || !d_out2 || B < 1 || T < 1 || V < 1 || L < T + 1) return kzv_fail(KZV_E_ARG, "target_weight_sum: bad argument");
    hipLaunchKernelGGL(target_weight_sum_kernel, dim3(1), dim3(1024), 0, s, labels, L, B, T, V, pad, d_class_weights, d_out2);
    return kzv_check_launch("target_weight_sum");
}

extern "C" int kzv_target_weight_sum(const int64_t* labels, int L, int B, int T, int V, int pad, const float* d_class_weights, float* d_out2, void* stream) {
    return kzv_target_weight_sum(labels, L, B, T, V, pad, d_class_weights, d_out2, (hipStream_t)stream);
}

// class weights and / or the focal exponent; neither: kzv_ce_fwd_bwd_ls itself, norm2[0] in the place of count
extern "C" int kzv_ce_fwd_bwd_w(const float* logits, int64_t ldl, const int64_t* labels, int L, int B, int T, int V, int pad,
                                const float* norm2, float* loss, void* dlogits_bf16, float label_smoothing, const float* d_class_weights,
                                float focal_gamma, void* stream) {
    return kzv_ce_fwd_bwd(logits, ldl, labels, L, B, T, V, pad, norm2, loss, (bf16_t*)dlogits_bf16, label_smoothing, (hipStream_t)stream, d_class_weights, focal_gamma);
}
