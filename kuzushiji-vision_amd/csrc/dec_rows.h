// What the decoder's ROW-PANEL kernels share (decoder_chain.hip: the forward chains; decoder_chain_bwd.hip: the input-gradient GEMMs and
// the backward segments; cross_entropy.hip: the one-launch LM head), each stated once.  One workgroup of 8 waves takes 64 rows through a
// chain of 256- / 768-wide GEMMs: operands in LDS, the weights as one fragment-order stream per wave (frag_stream.h), every tensor out
// through an LDS tile as whole rows.  Device-only; the unnamed namespace keeps each unit's copies (and its stamp array) its own.
#pragma once
#include "kzv_common.h"
#include "frag_stream.h"

namespace {

constexpr int HD = 256, FD = 768, RM = 64, RT = RM / 16;
constexpr int LDH = HD + 8;          // bf16 rows, 256 wide
constexpr int LDW = FD + 8;          // bf16 rows, 768 wide
constexpr int LDS_ = HD + 4;         // fp32 rows of a pre-LayerNorm sum
constexpr int NW = 8, WIN = 16;      // waves on the weight stream, fragments in flight per wave (frag_stream.h has the layout and the primitives)
constexpr int LDS_A1 = RM * LDH * 2;                                   // bytes of the 256-wide operand tile
constexpr int lds_max(int a, int b) { return a > b ? a : b; }         // for the dynamic-LDS sizes stated beside each kernel

// acc[c][rt][r] = sum_k W[n][k] * a[m][k],  m = 16 rt + (lane & 15),  n = (w + 8 c) * 16 + 4 (lane >> 4) + r
// NEXT (compile time): refill the window from `next` behind the last fragments -- no run-time branch around a load (see pin)
template <int CB, int KS, int NCB, int NKS, bool NEXT>
__device__ __forceinline__ void chain_gemm(bf16x8 (&R)[WIN], const char* wb, const char* next, const bf16_t* a_lds, int lda, int lane, f32x4 (&acc)[CB][RT]) {
    constexpr int F = CB * KS;
    static_assert(F % WIN == 0 && NCB * NKS >= WIN, "chain_gemm: window");
    const int l15 = lane & 15, g = lane >> 4;
    const unsigned wo = (unsigned)lane * 16u;
    const bf16_t* ap = a_lds + l15 * lda + g * 8;
#pragma unroll
    for (int c = 0; c < CB; ++c)
#pragma unroll
        for (int rt = 0; rt < RT; ++rt) acc[c][rt] = (f32x4){0.f, 0.f, 0.f, 0.f};
    bf16x8 fa[RT];
#pragma unroll
    for (int i = 0; i < F; ++i) {
        const int ks = i / CB, c = i % CB;
        if (c == 0) {
#pragma unroll
            for (int rt = 0; rt < RT; ++rt) fa[rt] = *(const bf16x8*)(ap + rt * 16 * lda + ks * 32);
        }
#pragma unroll
        for (int rt = 0; rt < RT; ++rt) acc[c][rt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(R[i % WIN], fa[rt], acc[c][rt], 0, 0, 0);
        if (i + WIN < F) R[i % WIN] = ld_frag<CB, KS, NW>(wb, wo, i + WIN);
        else if constexpr (NEXT) R[i % WIN] = ld_frag<NCB, NKS, NW>(next, wo, i + WIN - F);
    }
}

// Diagnostic build (-DKZV_STAMPS): the phase timeline of workgroup 0 of a unit's last launch.  No relocatable device code: each unit that
// stamps has an array of its own and reads it back through an entry of its own (decoder_chain.hip: dec_chain_b, slots 0 - 11,
// tools/dev/stamps_chain.py; decoder_chain_bwd.hip: dec_bwd_seg, slots 16 - 23, tools/dev/stamps_seg.py).
#ifdef KZV_STAMPS
__device__ long long g_chain_stamps[32];
#define CH_STAMP(k) do { if (blockIdx.x == 0 && threadIdx.x == 0) g_chain_stamps[k] = (long long)__builtin_amdgcn_s_memtime(); } while (0)
#ifndef KZV_STAMP_SEG_KS1
#define KZV_STAMP_SEG_KS1 8
#define KZV_STAMP_SEG_NP2 1
#endif
#define SEG_STAMP(k) do { if (KS1 == KZV_STAMP_SEG_KS1 && NP2 == KZV_STAMP_SEG_NP2) CH_STAMP(k); } while (0)
#else
#define CH_STAMP(k)
#define SEG_STAMP(k)
#endif

struct Drop { unsigned thr16; float inv_keep; unsigned key; };
// The residual operand of a "dropout(linear) + residual" epilogue: a stored fp32 tensor x, or -- when x is null -- the LayerNorm output
// it would hold, recomputed from that LayerNorm's INPUT sum s, its row statistics st = (mean, rstd) and its weights (the arithmetic of
// ln_rows / ln_fwd_kernel, so the same bits): the fp32 LayerNorm outputs of a decoder layer are read by nothing but the next residual,
// so the chains do not write them (3 x 15.7 MB per layer at 15k rows).
struct Resid { const float* x; const float* s; const float* st; const float* g; const float* b; };

// ---- tile movers ----------------------------------------------------------------------------------------------------------------------
// These are the movers the forward chains and the LM head share.  The backward kernels (decoder_chain_bwd.hip) spell their own loads and
// exits: their index arithmetic differs (signed division where load_rows shifts), and a second caller of a mover moves hipcc's schedule of
// the first -- tools/isa_diff.py --strict is the gate of any change here ("deliberately left duplicated").

// 64 rows x 256 bf16 columns, global -> LDS rows of LDH (rows past M read as zeros): the forward chains and the LM head
__device__ __forceinline__ void load_rows(const bf16_t* __restrict__ src, bf16_t* dst, int m0, int M, int tid) {
#pragma unroll
    for (int q = 0; q < RM * 32 / 512; ++q) {
        const int idx = tid + q * 512, row = idx >> 5, ch = idx & 31;
        uint4 v = make_uint4(0, 0, 0, 0);
        if (m0 + row < M) v = *(const uint4*)(src + (int64_t)(m0 + row) * HD + ch * 8);
        *(uint4*)(dst + row * LDH + ch * 8) = v;
    }
}
// bf16 output of a GEMM with CB column blocks per wave into an LDS tile: t[row][n] = acc + bias
template <int CB>
__device__ __forceinline__ void bf16_to_lds(const f32x4 (&acc)[CB][RT], const float* __restrict__ bias, bf16_t* t, int ldt, int w, int lane) {
    const int l15 = lane & 15, g = lane >> 4;
#pragma unroll
    for (int c = 0; c < CB; ++c) {
        const int n0 = (w + 8 * c) * 16 + 4 * g;
        const float4 bb = *(const float4*)(bias + n0);
#pragma unroll
        for (int rt = 0; rt < RT; ++rt)
            *(uint2*)(t + (rt * 16 + l15) * ldt + n0) = make_uint2(pack_bf2(acc[c][rt][0] + bb.x, acc[c][rt][1] + bb.y), pack_bf2(acc[c][rt][2] + bb.z, acc[c][rt][3] + bb.w));
    }
}
// the backward of GELU on four adjacent columns: times the forward's saved gelu'(pre-activation) (bf16 x 4), as nt_emit<KZV_EPI_DGELU>
__device__ __forceinline__ void scale_by_bf16x4(f32x4& v, const uint2 u) {
    v[0] *= bf2f((bf16_t)(u.x & 0xffff)); v[1] *= bf2f((bf16_t)(u.x >> 16)); v[2] *= bf2f((bf16_t)(u.y & 0xffff)); v[3] *= bf2f((bf16_t)(u.y >> 16));
}
// an LDS tile of 64 rows x NCH 16-byte pieces -> global rows of ldo elements (whole rows, 16 bytes per lane)
template <int NCH>
__device__ __forceinline__ void rows_out(const bf16_t* t, int ldt, bf16_t* __restrict__ out, int64_t ldo, int m0, int M, int tid) {
#pragma unroll
    for (int q = 0; q < RM * NCH / 512; ++q) {
        const int idx = tid + q * 512, row = idx / NCH, ch = idx - row * NCH;
        if (m0 + row < M) *(uint4*)(out + (int64_t)(m0 + row) * ldo + ch * 8) = *(const uint4*)(t + row * ldt + ch * 8);
    }
}

// ---- the "dropout(linear) + residual" epilogue and the LayerNorm behind it --------------------------------------------------------------
// "dropout(linear) + residual" epilogue of a 256-wide GEMM: s = drop(acc + bias) + resid -> the LDS sum tile.  (Nothing goes to
// global memory from the MFMA layout -- a lane holds 4 columns of 16 different rows there, i.e. 32- / 64-byte pieces of 16 rows per
// store instruction, which is what made the first version of these kernels 2.7x slower than its byte count: every tensor leaves
// through an LDS tile as whole rows.)
// The epilogue's global operands (residual rows in the MFMA layout: 64-byte pieces of 16 rows per instruction, plus the row statistics when
// the residual is recomputed) are requested BEFORE the GEMM whose result they meet -- behind it they were 6 - 8 k cycles of exposed latency
// per epilogue (tools/dev/stamps_chain.py).  Rows past M read the last row (never used).
// THE HAZARD IDIOM OF THIS FAMILY.  Registers loaded long before their use are retired BY HAND: `s_waitcnt vmcnt(0)` and then every such
// register through an empty asm, so that no use can be scheduled above the wait (volatile asms keep their order; plain arithmetic does not
// stay behind one).  hipcc's own count is not enough here: with loads inside uniform branches (the residual's statistics) between the load
// and its use, the wait it emitted let the use run first -- chain A read rstd = 0 (the register's initial value) in 2 - 5 % of its
// workgroups once the launch had more workgroups than CUs (slower loads), i.e. residual = beta for 16 rows (tools/dev/r5_det3.py; rounds
// 3 - 4 before this).  Users: resid_epilogue below; dec_bwd_seg_kernel (the LayerNorm backward's operands, the saved gelu').
__device__ __forceinline__ void pin(float& f) { asm volatile("" : "+v"(f)); }
__device__ __forceinline__ void pin(unsigned& f) { asm volatile("" : "+v"(f)); }
__device__ __forceinline__ void pin(float4& v) { pin(v.x); pin(v.y); pin(v.z); pin(v.w); }
__device__ __forceinline__ void pin(float2& v) { pin(v.x); pin(v.y); }
__device__ __forceinline__ void pin(uint2& v) { pin(v.x); pin(v.y); }
__device__ __forceinline__ void retire_loads() { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }
struct ResidRegs { float4 v[2][RT]; float2 st[RT]; };
__device__ __forceinline__ void resid_prefetch(const Resid& resid, ResidRegs& r, int m0, int M, int w, int lane) {
    const int l15 = lane & 15, g = lane >> 4;
    const float* src = resid.x ? resid.x : resid.s;
    const float* stp = resid.x ? resid.x : resid.st;         // no branch around a load: a stored residual reads two of its own floats here (unused)
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) {
        const int64_t m = min(m0 + rt * 16 + l15, M - 1);
#pragma unroll
        for (int c = 0; c < 2; ++c) r.v[c][rt] = *(const float4*)(src + m * HD + (w + 8 * c) * 16 + 4 * g);
        r.st[rt] = *(const float2*)(stp + 2 * m);
    }
}
__device__ __forceinline__ void resid_epilogue(const f32x4 (&acc)[2][RT], const float* __restrict__ bias, const Resid& resid, const ResidRegs& pre_in, const Drop& d,
                                               float* s_lds, int m0, int M, int w, int lane) {
    const int l15 = lane & 15, g = lane >> 4;
    ResidRegs pre = pre_in;                                   // requested one GEMM ago: retired by hand (see pin)
    retire_loads();
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) { pin(pre.v[0][rt]); pin(pre.v[1][rt]); pin(pre.st[rt]); }
#pragma unroll
    for (int c = 0; c < 2; ++c) {
        const int n0 = (w + 8 * c) * 16 + 4 * g;
        const float4 bb = *(const float4*)(bias + n0);
#pragma unroll
        for (int rt = 0; rt < RT; ++rt) {
            const int row = rt * 16 + l15, m = m0 + row;
            if (m < M) {
                float v[4] = {acc[c][rt][0] + bb.x, acc[c][rt][1] + bb.y, acc[c][rt][2] + bb.z, acc[c][rt][3] + bb.w};
                if (d.thr16) KZV_DROP4(v[0], v[1], v[2], v[3], d.key, (unsigned)m * (unsigned)HD + (unsigned)n0, d.thr16, d.inv_keep);
                float4 x4;
                if (resid.x) x4 = pre.v[c][rt];
                else {
                    const float4 sv = pre.v[c][rt], gm = *(const float4*)(resid.g + n0), bt = *(const float4*)(resid.b + n0);
                    const float mean = pre.st[rt].x, rstd = pre.st[rt].y;
                    const float a0 = sv.x - mean, a1 = sv.y - mean, a2 = sv.z - mean, a3 = sv.w - mean;
                    x4 = make_float4(a0 * rstd * gm.x + bt.x, a1 * rstd * gm.y + bt.y, a2 * rstd * gm.z + bt.z, a3 * rstd * gm.w + bt.w);
                }
                *(float4*)(s_lds + row * LDS_ + n0) = make_float4(v[0] + x4.x, v[1] + x4.y, v[2] + x4.z, v[3] + x4.w);
            }
        }
    }
}
// LayerNorm of the 64 sum rows (wave w: rows 8 w .. 8 w + 7; a row = one KiB per store), the arithmetic of ln_fwd_kernel: the sum s,
// x (fp32) and xh (bf16) to global, xh also to the LDS operand tile, (mean, rstd) to stats
__device__ __forceinline__ void ln_rows(const float* s_lds, const float* __restrict__ gamma, const float* __restrict__ beta, float eps, float* __restrict__ s_out,
                                        float* __restrict__ x_out, bf16_t* __restrict__ xh_out, float* __restrict__ stats, bf16_t* a_lds, int m0, int M, int w, int lane) {
    constexpr int NR = RM / 8;
    const float4 gm = *(const float4*)(gamma + lane * 4), bt = *(const float4*)(beta + lane * 4);
    float4 v8[NR];              // every row out of LDS before the first LDS store below: hipcc cannot tell the sum tile from the operand tile and
#pragma unroll                  // would otherwise keep each row's LDS read behind the previous row's write
    for (int q = 0; q < NR; ++q) v8[q] = *(const float4*)(s_lds + (w * NR + q) * LDS_ + lane * 4);
    // The two wave reductions of a row are 12 dependent ds_bpermute round trips (~120 cycles each): row by row that was 1.8 k cycles per
    // row, 14 k per LayerNorm phase (tools/dev/stamps_chain.py).  The eight rows of a wave are independent, so each butterfly step is
    // taken for all of them together -- the same additions in the same order per row (wave_sum's), eight shuffles in flight at a time.
    float t8[NR], mean8[NR], rstd8[NR];
#pragma unroll
    for (int q = 0; q < NR; ++q) t8[q] = v8[q].x + v8[q].y + v8[q].z + v8[q].w;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        float u8[NR];
#pragma unroll
        for (int q = 0; q < NR; ++q) u8[q] = __shfl_xor(t8[q], o, 64);
#pragma unroll
        for (int q = 0; q < NR; ++q) t8[q] += u8[q];
    }
    float4 c8[NR];
#pragma unroll
    for (int q = 0; q < NR; ++q) {
        mean8[q] = t8[q] / (float)HD;
        c8[q] = make_float4(v8[q].x - mean8[q], v8[q].y - mean8[q], v8[q].z - mean8[q], v8[q].w - mean8[q]);
        t8[q] = c8[q].x * c8[q].x + c8[q].y * c8[q].y + c8[q].z * c8[q].z + c8[q].w * c8[q].w;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        float u8[NR];
#pragma unroll
        for (int q = 0; q < NR; ++q) u8[q] = __shfl_xor(t8[q], o, 64);
#pragma unroll
        for (int q = 0; q < NR; ++q) t8[q] += u8[q];
    }
#pragma unroll
    for (int q = 0; q < NR; ++q) rstd8[q] = rsqrtf(t8[q] / (float)HD + eps);
#pragma unroll
    for (int q = 0; q < NR; ++q) {
        const int row = w * NR + q, m = m0 + row;
        if (m >= M) {                                 // wave-uniform
            *(uint2*)(a_lds + row * LDH + lane * 4) = make_uint2(0, 0);
            continue;
        }
        const float4 v = v8[q];
        *(float4*)(s_out + (int64_t)m * HD + lane * 4) = v;
        const float mean = mean8[q], rstd = rstd8[q];
        const float a = c8[q].x, b = c8[q].y, c = c8[q].z, d = c8[q].w;
        if (lane == 0) { stats[2 * (int64_t)m] = mean; stats[2 * (int64_t)m + 1] = rstd; }
        const float o0 = a * rstd * gm.x + bt.x, o1 = b * rstd * gm.y + bt.y, o2 = c * rstd * gm.z + bt.z, o3 = d * rstd * gm.w + bt.w;
        const uint2 h = make_uint2(pack_bf2(o0, o1), pack_bf2(o2, o3));
        if (x_out) *(float4*)(x_out + (int64_t)m * HD + lane * 4) = make_float4(o0, o1, o2, o3);
        *(uint2*)(xh_out + (int64_t)m * HD + lane * 4) = h;
        *(uint2*)(a_lds + row * LDH + lane * 4) = h;
    }
}

}  // namespace
