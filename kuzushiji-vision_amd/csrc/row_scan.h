// One wave over one fp32 logits row: what token_scores_kernel (attention_probs.hip) and the top-k kernels (token_topk.hip) share.
// Each lane scans its columns in ascending order and keeps the maximum, its first column and the sum of exp(x - max) under that maximum
// (rescaled when the maximum moves); the lanes are then combined by xor shuffles under the row maximum -- a fixed order, so the
// log-sum-exp is bit-reproducible and the same number in both kernels.
#pragma once
#include "kzv_common.h"

constexpr int ROW_NO_COL = 0x7fffffff;                       // "no column yet": loses every tie

struct RowScan {
    float mx = -INFINITY, se = 0.f;
    int arg = ROW_NO_COL;
    __device__ __forceinline__ void take(float x, int col) {
        if (x > mx) { se *= __expf(mx - x); mx = x; arg = col; }      // ascending columns: strict > keeps the first
        if (mx > -INFINITY) se += __expf(x - mx);                     // (a -inf column before any finite one adds nothing)
    }
};

// does (value ov, column oc) rank before (v, c)?  The larger value, the smaller column among equals (the FIRST arg-max)
__device__ __forceinline__ bool row_before(float ov, int oc, float v, int c) { return ov > v || (ov == v && oc < c); }

// the best (value, column) of the wave's 64 candidates, in every lane
__device__ __forceinline__ void wave_first_argmax(float& v, int& c) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float ov = __shfl_xor(v, o, 64);
        const int oc = __shfl_xor(c, o, 64);
        if (row_before(ov, oc, v, c)) { v = ov; c = oc; }
    }
}

// log-sum-exp of the row from the lanes' scans, mx = the row maximum (wave_first_argmax of their st.mx)
__device__ __forceinline__ float wave_lse(const RowScan& st, float mx) {
    const float se = wave_sum(st.arg == ROW_NO_COL ? 0.f : st.se * __expf(st.mx - mx));
    return mx + __logf(se);
}
