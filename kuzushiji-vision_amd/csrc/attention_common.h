// What the attention kernel files (attention.hip, attention_d96.hip, attention_stream.hip, attention_generic.hip) and their
// dispatch (attention_api.cpp) share, each stated once.  Most of it is CONTRACT, not convenience: the LDS image layout must agree
// between the code that stages an image and the code that reads it, and the dropout bookkeeping must agree bit for bit between
// every kernel (a forward of one file is differentiated by a backward of the same family) and with oracle/attn_dropout.py.
//
// A translation unit that wants the streaming hint on its LDS-DMA defines KZV_GLDS_NT BEFORE including this header (it pulls in
// kzv_common.h, which is #pragma once: a later define would silently be ignored).
#pragma once
#include "kzv_common.h"
#include "../../include/kzv.h"
#include "kzv_host.h"

// ---- limits (kernel files, dispatch, model.cpp) -----------------------------------------------------------------------
constexpr int KZV_ATTN_MAX_S = 288;             // whole-head MFMA kernels: one head's K and V resident in LDS
constexpr int KZV_ATTN_MAX_CAUSAL = 192;        // ... in causal mode (the <= 12-tile instances)
constexpr int KZV_ATTN_STREAM_MAX_S = 4097;     // K/V-streaming kernels: 4,096 patches + CLS
constexpr int KZV_ATTN_VALU_MAX_SK = 512;       // the VALU kernel holds 8 keys per lane

// ---- internal launches: the caller has chosen AND validated the implementation (attention_api.cpp) --------------------
int kzv_attn_mfma64(const kzv_attn_args* a, bool bwd, hipStream_t s);                 // attention.hip
int kzv_attn_d96(const kzv_attn_args* a, bool bwd, hipStream_t s);                    // attention_d96.hip
int kzv_attn_stream(const kzv_attn_args* a, bool bwd, hipStream_t s);                 // attention_stream.hip (head_dim 96, else 64)
int kzv_attn_generic(const kzv_attn_args* a, int D, bool bwd, hipStream_t s);         // attention_generic.hip
size_t kzv_attn_generic_lds(int D, int Sk);                                           // ... and the LDS bytes it would ask for
int kzv_attn_stream_check(const kzv_attn_args* a, bool bwd);                          // what the streaming kernels refuse
// launches implementation `impl` (KZV_ATTN_MFMA64 / _MFMA96 / _VALU / _STREAM64 / _STREAM96) inside the profiling scope of its
// path (class 2 forward, 3 backward)
int kzv_attn_launch(const kzv_attn_args* a, int impl, bool bwd, hipStream_t s);

// The fields every kernel parameter block has in common.  The blocks share this filler, NOT a layout: widening AttnP96 by the
// three ids fields of AttnP changed the kernel-argument loads and the instruction order of both head_dim-96 kernels.
template <class P>
void kzv_attn_fill(P& p, const kzv_attn_args* a, int D) {
    p.Q = (const bf16_t*)a->Q; p.K = (const bf16_t*)a->K; p.V = (const bf16_t*)a->V; p.O = (bf16_t*)a->O; p.LSE = a->LSE;
    p.dO = (const bf16_t*)a->dO; p.dQ = (bf16_t*)a->dQ; p.dK = (bf16_t*)a->dK; p.dV = (bf16_t*)a->dV;
    p.ldq = a->ldq; p.ldk = a->ldk; p.ldv = a->ldv; p.ldo = a->ldo;
    p.B = a->B; p.heads = a->heads; p.Sq = a->Sq; p.Sk = a->Sk;
    p.scale = D == 64 ? 0.125f : 1.f / sqrtf((float)D);     // head_dim^-0.5 in fp32: every kernel of the family and the oracle
    kzv_drop_params(a->drop_p, &p.thr16, &p.inv_keep);
    p.key = a->drop_key;
}
// ... and the zero page behind the rows past the end of an LDS image (the MFMA kernels)
template <class P>
int kzv_attn_fill_zero(P& p, const char* who) {
    p.zero16 = kzv_zero_page();
    return p.zero16 ? KZV_OK : kzv_fail(KZV_E_HIP, "%s: zero page unavailable", who);
}

// ---- small device helpers ---------------------------------------------------------------------------------------------
constexpr float LOG2E = 1.4426950408889634f;
typedef __attribute__((ext_vector_type(4))) unsigned u32x4;
__device__ __forceinline__ bf16x8 cat8(bf16x4 a, bf16x4 b) { return (bf16x8){a[0], a[1], a[2], a[3], b[0], b[1], b[2], b[3]}; }
__device__ __forceinline__ bf16x8 words8(unsigned a, unsigned b, unsigned c, unsigned d) { return __builtin_bit_cast(bf16x8, (u32x4){a, b, c, d}); }
__device__ __forceinline__ float fmax3(float a, float b, float c) { return __builtin_fmaxf(__builtin_fmaxf(a, b), c); }
// d + a . b, accumulated in element order (the order is part of the result)
__device__ __forceinline__ float dot8(bf16x8 a, bf16x8 b, float d = 0.f) {
#pragma unroll
    for (int j = 0; j < 8; ++j) d += bf2f((bf16_t)a[j]) * bf2f((bf16_t)b[j]);
    return d;
}
// Values loaded before a sweep are "used" here, after the prologue's vmcnt(0): hipcc cannot see the asm LDS-DMAs, so a first
// use inside the sweep would get a compiler wait (vmcnt(0)..(3)) that also drains the next block's DMA issued in the same
// iteration.  With every prologue load consumed up front, the loops carry no vmcnt but the one per block.
__device__ __forceinline__ void pin(bf16x8& v) { asm volatile("" : "+v"(v)); }
__device__ __forceinline__ void pin(u32x4& v) { asm volatile("" : "+v"(v)); }
__device__ __forceinline__ void pin(float& v) { asm volatile("" : "+v"(v)); }
__device__ __forceinline__ void pin(AttDropLane& d) { asm volatile("" : "+v"(d.c01), "+v"(d.c23), "+v"(d.m01), "+v"(d.m23), "+v"(d.rot)); }
// four accumulators (consecutive columns of one output row) scaled and stored as bf16
__device__ __forceinline__ void store_bf4(bf16_t* dst, f32x4 a, float sc) {
    *(uint2*)dst = make_uint2(pack_bf2(a[0] * sc, a[1] * sc), pack_bf2(a[2] * sc, a[3] * sc));
}

// ---- LDS image of a [rows][D] bf16 operand ------------------------------------------------------------------------------
// Rows of 2 D bytes in 16-byte chunks; chunk c of row r sits at slot c ^ swz(r).  D = 64 (128-byte rows): swz = r & 7.  D = 96
// (192-byte rows, 12 chunks): the two bits (r >> 2) & 3 swapped, which keeps c >> 2, so chunk groups 4 i and 16-column tiles
// dt, dt + 2, dt + 4 are immediates.  Row reads (16 rows, one chunk) and transposed reads (4-row blocks at rows 4g + q of a
// 16-aligned base, 2 chunks) are both conflict-free.
template <int D> __device__ __forceinline__ int swz(int r) {
    if constexpr (D == 64) return r & 7;
    else return (((r >> 2) & 1) << 1) | ((r >> 3) & 1);
}
template <int D> __device__ __forceinline__ int img_off(int r, int c) { return r * (2 * D) + ((c ^ swz<D>(r)) << 4); }
// per-lane offset of a transposed read: block rows 4g .. 4g + 3 (+ a 16-aligned base), 16 columns from chunk 2 * dt
template <int D> __device__ __forceinline__ int tr_off(int g, int l15, int dt) {
    const int r = 4 * g + (l15 >> 2);
    return img_off<D>(r, 2 * dt + ((l15 >> 1) & 1)) + (l15 & 1) * 8;
}

// ---- dropout bookkeeping (generator: kzv_common.h; numpy statement: oracle/attn_dropout.py) ---------------------------------
// 4-wide blocks along a sequence of S.  A macro: as an inline function, the same expression left every backward kernel of
// attention.hip with three more v_mul_lo_u32 and two more VGPRs (the early passes run before the inliner).
#define KZV_ATT_N4(S) ((unsigned)((S) + 3) >> 2)
// index of the 4 x 4 block (q >> 2 = q4, k >> 2 = k4) of pair bh = b * heads + h
__device__ __forceinline__ unsigned att_block(unsigned bh, unsigned nQ4, unsigned q4, unsigned nK4, unsigned k4) { return (bh * nQ4 + q4) * nK4 + k4; }
// its pre-mix word; a step of one block along k adds KZV_ATT_GOLD, one along q adds nK4 * KZV_ATT_GOLD
__device__ __forceinline__ unsigned att_block_word(unsigned bh, unsigned nQ4, unsigned q4, unsigned nK4, unsigned k4, unsigned key) {
    return att_block(bh, nQ4, q4, nK4, k4) * KZV_ATT_GOLD + key;
}
// forward threshold for att_keep_mask: two copies of (int16)(thr16 - 32768 - 1)
__device__ __forceinline__ unsigned att_thrm1x2(unsigned thr16) { return (unsigned)((thr16 - 32768 - 1) & 0xffff) * 0x10001u; }
// backward threshold, compared as int16 >= thr_s; no dropout: below every int16, everything is kept
__device__ __forceinline__ int att_thr_s(unsigned thr16) { return thr16 ? (int)thr16 - 32768 : -40000; }

// ---- backward: one element ------------------------------------------------------------------------------------------------
// Element r = 0..3 of a lane's piece: four consecutive queries of its key (dK / dV orientation) or keys of its query (dQ).
// P = exp2(S * sc - lse), lse in log2 units (+inf for rows past Sq and dead rows: P = 0), forced to 0 where MASKED and not ok;
// kept P = P where the element's 16-bit dropout value (a half of u01 | u23 of att_drop_u) is >= thr_s; dS = kept P * dP - P * delta'.
// 1 / P(keep) is not applied here: delta' carries P(keep) and the outputs are scaled at the very end.
template <bool MASKED>
__device__ __forceinline__ void att_bwd_elem(int r, float s, float dp, float sc, float lse, float delta, bool ok, unsigned u01, unsigned u23, int thr_s,
                                             float& pkept, float& ds) {
    float pr = __builtin_amdgcn_exp2f(fmaf(s, sc, -lse));
    if (MASKED) pr = ok ? pr : 0.f;
    const unsigned ur = (r & 2) ? u23 : u01;
    const int us = (r & 1) ? (int)ur >> 16 : (int)(short)(ur & 0xffffu);
    pkept = us >= thr_s ? pr : 0.f;
    ds = fmaf(pkept, dp, -pr * delta);
}

// ---- forward: one key tile ------------------------------------------------------------------------------------------------
// Four consecutive keys of the lane's query, in place: s <- P = exp2(S * sc - mref) (un-normalised; added to the row sum), packed as
// two bf16 pairs into pw[0..1] with the dropped elements zeroed.  xw is the pre-mix word of the tile's 4 x 4 block (att_block_word),
// thrm1x2 = att_thrm1x2(thr16).  `sum` must name a scalar local: with the array element l[it] of stream_fwd_kernel<96> bound to
// it, that kernel was allocated 160 VGPRs instead of 206, with six more s_waitcnt.
__device__ __forceinline__ void att_fwd_tile(f32x4& s, float sc, float mref, float& sum, unsigned thr16, const AttDropLane& dl, unsigned xw,
                                              unsigned thrm1x2, unsigned* pw) {
#pragma unroll
    for (int r = 0; r < 4; ++r) { s[r] = __builtin_amdgcn_exp2f(fmaf(s[r], sc, -mref)); sum += s[r]; }
    unsigned w01 = pack_bf2(s[0], s[1]), w23 = pack_bf2(s[2], s[3]);
    if (thr16) {
        unsigned u01, u23;
        att_drop_u(dl, att_mix(xw), &u01, &u23);
        w01 &= att_keep_mask(u01, thrm1x2); w23 &= att_keep_mask(u23, thrm1x2);
    }
    pw[0] = w01; pw[1] = w23;
}

// ---- backward prologue: log-sum-exp and delta' of one query row, four lanes per row ----------------------------------------------
// d = this lane's quarter of rowsum(dO . O) (dot8 over its chunks), lv = the row's natural-log LSE.  Writes lse[row] in log2 units
// and delta' = rowsum * P(keep) (1 / P(keep) is taken out of dS and multiplied back into dQ / dK / dV at the very end); rows in
// [Sq, nrows) get +inf and 0, so P = dS = 0 there whatever the (clamped, finite) operand rows hold.
__device__ __forceinline__ void att_row_stats(float d, float lv, float keep_p, int row, int nrows, int Sq, int tid, float* lse, float* dlt) {
    d += __shfl_xor(d, 1, 64);
    d += __shfl_xor(d, 2, 64);
    if ((tid & 3) == 0 && row < nrows) {
        lse[row] = row < Sq ? lv * LOG2E : INFINITY;
        dlt[row] = row < Sq ? d * keep_p : 0.f;
    }
}
