// The linear chains of a RoBERTa decoder layer in the TRAINING forward (HF modeling_roberta.py:421-464 under
// src/models/trocr_model.py:258-297), two launches per layer instead of nine:
//   A (between the two attentions):  s1 = drop(ctx Wo^T + b) + x;  x1 = LN1(s1);  cq = x1 Wcq^T + b
//   B (after the cross-attention):   s2 = drop(cctx Wco^T + b) + x1;  x2 = LN2(s2);  act = gelu(x2 Wfc1^T + b);
//                                    s3 = drop(act Wfc2^T + b) + x2;  x3 = LN3(s3);  [qkv of the NEXT layer = x3 Wqkv^T + b]
// At the decoder's size (hidden 256, FFN 768, ~15k rows) every one of these is a 15 - 21 us launch for 2 GFLOP: 240 tiles of
// 128 x 128 leave the chip under one wave per SIMD and the chain is launch- and latency-bound.  The chains are ROW-LOCAL, so one
// workgroup takes 64 rows through a whole chain: the activations stay in LDS (bf16 A operands, fp32 pre-LayerNorm sums), the
// weights arrive in MFMA fragment order (frag_stream.h, shared with decode_fused.hip: a wave-instruction = one contiguous KiB) as one stream per wave
// with a window of 16 fragments in flight across the GEMM boundaries, and every tensor the backward reads is written on the way
// (same tensors, same rounding points as the launch-per-operation path: bf16 GEMM operands, fp32 sums / statistics / residuals;
// the dropout bits of the two residual epilogues are the engine's own -- key, element index m * 256 + n -- so the backward's
// regenerated masks match).  Each weight fragment feeds four MFMAs (the four 16-row tiles).
// The family's shared pieces (chain_gemm, the tile movers, the residual epilogue, ln_rows, the pin / retire_loads idiom) are dec_rows.h;
// the backward of these chains is decoder_chain_bwd.hip, the LM head cross_entropy.hip, the weight packer frag_pack.hip.
#include "dec_rows.h"
#include "../../include/kzv.h"
#include "kzv_host.h"
#include "kzv_kernels.h"

namespace {

constexpr int LDS_A = LDS_A1 + RM * LDS_ * 4, LDS_B = LDS_A1 + RM * LDW * 2;      // dec_chain_a: operand + sum tile; dec_chain_b: operand + activation tile
static_assert(LDS_A == 100352 && LDS_B == 133120, "dec_chain: dynamic LDS");

struct SegA {
    const bf16_t* ctx; Resid xres; const bf16_t* wo; const float* bo; Drop drop; const float *g1, *b1; const bf16_t* wcq; const float* bcq;
    float* s1; float* st1; float* x1; bf16_t* x1h; bf16_t* cq; int M; float eps;
};
struct SegB {
    const bf16_t* cctx; Resid x1; const bf16_t* wco; const float* bco; Drop drop3; const float *g2, *b2;
    const bf16_t* wfc1; const float* bfc1; const bf16_t* wfc2; const float* bfc2; Drop drop4; const float *g3, *b3;
    const bf16_t* wqkv; const float* bqkv;                       // the next layer's QKV projection, or null
    float *s2, *st2, *x2; bf16_t* x2h; bf16_t *pre, *act; float *s3, *st3, *x3; bf16_t* x3h; bf16_t* qkv;
    int M; float eps;
};

__global__ __launch_bounds__(512) void dec_chain_a_kernel(const SegA p) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    bf16_t* a1 = (bf16_t*)smem;                                   // [RM][LDH] bf16 operand tile
    float* ssum = (float*)(smem + LDS_A1);                        // [RM][LDS_] pre-LayerNorm sums
    const int tid = threadIdx.x, lane0 = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int m0 = blockIdx.x * RM;
    bf16x8 R[WIN];
    fill_window<2, 8, NW, WIN>(R, wave_frags<2, 8>(p.wo, w), opaque(lane0));
    load_rows(p.ctx, a1, m0, p.M, opaque(tid));
    ResidRegs rr;
    resid_prefetch(p.xres, rr, m0, p.M, w, opaque(lane0));
    wg_barrier();
    {
        const int lane = opaque(lane0);
        f32x4 acc[2][RT];
        chain_gemm<2, 8, 2, 8, true>(R, wave_frags<2, 8>(p.wo, w), wave_frags<2, 8>(p.wcq, w), a1, LDH, lane, acc);
        resid_epilogue(acc, p.bo, p.xres, rr, p.drop, ssum, m0, p.M, w, lane);
    }
    wg_barrier();                // every wave has read the ctx tile and written its part of the sum tile
    ln_rows(ssum, p.g1, p.b1, p.eps, p.s1, p.x1, p.x1h, p.st1, a1, m0, p.M, w, opaque(lane0));
    wg_barrier();                // the sum tile is dead: it stages the cross query
    {
        const int lane = opaque(lane0);
        f32x4 acc[2][RT];
        chain_gemm<2, 8, 2, 8, false>(R, wave_frags<2, 8>(p.wcq, w), nullptr, a1, LDH, lane, acc);
        bf16_to_lds<2>(acc, p.bcq, (bf16_t*)ssum, LDH, w, lane);
    }
    wg_barrier();
    rows_out<32>((const bf16_t*)ssum, LDH, p.cq, HD, m0, p.M, opaque(tid));
}

__global__ __launch_bounds__(512) void dec_chain_b_kernel(const SegB p) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    bf16_t* a1 = (bf16_t*)smem;                                   // [RM][LDH] bf16 operand tile
    bf16_t* a2 = (bf16_t*)(smem + LDS_A1);                        // [RM][LDW] the FFN activation; the sum tiles alias it
    float* ssum = (float*)a2;
    static_assert(RM * LDS_ * 4 <= RM * LDW * 2, "the sum tile must fit the activation tile");
    const int tid = threadIdx.x, lane0 = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int m0 = blockIdx.x * RM;
    bf16x8 R[WIN];
    CH_STAMP(0);
    fill_window<2, 8, NW, WIN>(R, wave_frags<2, 8>(p.wco, w), opaque(lane0));
    load_rows(p.cctx, a1, m0, p.M, opaque(tid));
    ResidRegs rr;
    resid_prefetch(p.x1, rr, m0, p.M, w, opaque(lane0));
    wg_barrier();
    CH_STAMP(1);
    {   // s2 = drop(cctx Wco^T + b) + x1
        const int lane = opaque(lane0);
        f32x4 acc[2][RT];
        chain_gemm<2, 8, 6, 8, true>(R, wave_frags<2, 8>(p.wco, w), wave_frags<6, 8>(p.wfc1, w), a1, LDH, lane, acc);
        resid_epilogue(acc, p.bco, p.x1, rr, p.drop3, ssum, m0, p.M, w, lane);
    }
    wg_barrier();
    CH_STAMP(2);
    ln_rows(ssum, p.g2, p.b2, p.eps, p.s2, p.x2, p.x2h, p.st2, a1, m0, p.M, w, opaque(lane0));
    // s2 / st2 come back from global memory below (the fc2 epilogue's residual, read in the MFMA layout by OTHER waves than the ones that
    // stored them): the stores must have completed before the barrier that orders the two -- a workgroup barrier alone orders LDS only
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    wg_barrier();                // the sum tile is dead from here: the activation tile may be written
    CH_STAMP(3);
    {   // act = gelu(x2 Wfc1^T + b) -> the activation tile; the derivative (saved for the backward, KZV_EPI_GELU) leaves in three
        // passes of 256 columns through the operand tile, which the MFMAs no longer read
        const int lane = opaque(lane0), l15 = lane & 15, g = lane >> 4;
        f32x4 acc[6][RT];
        chain_gemm<6, 8, 2, 24, true>(R, wave_frags<6, 8>(p.wfc1, w), wave_frags<2, 24>(p.wfc2, w), a1, LDH, lane, acc);
        wg_barrier();            // every wave has read x2h
        CH_STAMP(4);
#pragma unroll
        for (int pass = 0; pass < 3; ++pass) {
#pragma unroll
            for (int cc = 0; cc < 2; ++cc) {
                const int c = 2 * pass + cc;
                const int n0 = (w + 8 * c) * 16 + 4 * g;
                const float4 bb = *(const float4*)(p.bfc1 + n0);
#pragma unroll
                for (int rt = 0; rt < RT; ++rt) {
                    const int row = rt * 16 + l15;
                    float y[4], d[4];
                    gelu_erf_both(acc[c][rt][0] + bb.x, &y[0], &d[0]); gelu_erf_both(acc[c][rt][1] + bb.y, &y[1], &d[1]);
                    gelu_erf_both(acc[c][rt][2] + bb.z, &y[2], &d[2]); gelu_erf_both(acc[c][rt][3] + bb.w, &y[3], &d[3]);
                    *(uint2*)(a2 + row * LDW + n0) = make_uint2(pack_bf2(y[0], y[1]), pack_bf2(y[2], y[3]));
                    *(uint2*)(a1 + row * LDH + n0 - 256 * pass) = make_uint2(pack_bf2(d[0], d[1]), pack_bf2(d[2], d[3]));
                }
            }
            wg_barrier();
            rows_out<32>(a1, LDH, p.pre + 256 * pass, FD, m0, p.M, opaque(tid));
            wg_barrier();
        }
    }
    CH_STAMP(5);
    rows_out<96>(a2, LDW, p.act, FD, m0, p.M, opaque(tid));       // (the last barrier above also covers the activation tile)
    CH_STAMP(6);
    f32x4 acc3[2][RT];
    const Resid res2{p.x2, p.s2, p.st2, p.g2, p.b2};              // x2: this workgroup's own rows, written above (ln_rows; many barriers ago)
    resid_prefetch(res2, rr, m0, p.M, w, opaque(lane0));
    {   // s3 = drop(act Wfc2^T + b) + x2
        const int lane = opaque(lane0);
        if (p.wqkv) chain_gemm<2, 24, 6, 8, true>(R, wave_frags<2, 24>(p.wfc2, w), wave_frags<6, 8>(p.wqkv, w), a2, LDW, lane, acc3);
        else chain_gemm<2, 24, 6, 8, false>(R, wave_frags<2, 24>(p.wfc2, w), nullptr, a2, LDW, lane, acc3);
    }
    wg_barrier();                // every wave has read the activation tile: the sum tile (same memory) may be written
    CH_STAMP(7);
    resid_epilogue(acc3, p.bfc2, res2, rr, p.drop4, ssum, m0, p.M, w, opaque(lane0));
    wg_barrier();
    CH_STAMP(8);
    ln_rows(ssum, p.g3, p.b3, p.eps, p.s3, p.x3, p.x3h, p.st3, a1, m0, p.M, w, opaque(lane0));
    CH_STAMP(9);
    if (!p.wqkv) return;
    wg_barrier();
    {   // the next layer's q | k | v = x3 Wqkv^T + b, staged through the (dead) activation tile
        const int lane = opaque(lane0);
        f32x4 acc[6][RT];
        chain_gemm<6, 8, 2, 8, false>(R, wave_frags<6, 8>(p.wqkv, w), nullptr, a1, LDH, lane, acc);
        bf16_to_lds<6>(acc, p.bqkv, a2, LDW, w, lane);
    }
    wg_barrier();
    CH_STAMP(10);
    rows_out<96>(a2, LDW, p.qkv, 3 * HD, m0, p.M, opaque(tid));
    CH_STAMP(11);
}

}  // namespace

#ifdef KZV_STAMPS
extern "C" int kzv_debug_chain_stamps(long long* host, int n) {
    return hipMemcpyFromSymbol(host, HIP_SYMBOL(g_chain_stamps), sizeof(long long) * (n < 32 ? n : 32)) == hipSuccess ? 0 : 1;
}
#endif

int kzv_dec_chain_supported(int Hd, int Fd) { return Hd == HD && Fd == FD; }

int kzv_dec_chain_a(const KzvDecChainA& a, hipStream_t s) {
    if (a.M < 1) return kzv_fail(KZV_E_ARG, "dec_chain_a: rows");
    SegA p;
    p.ctx = a.ctx; p.xres = Resid{a.xres, a.xres_s, a.xres_st, a.xres_g, a.xres_b}; p.wo = a.wo; p.bo = a.bo; p.g1 = a.g1; p.b1 = a.b1; p.wcq = a.wcq; p.bcq = a.bcq;
    p.s1 = a.s1; p.st1 = a.st1; p.x1 = a.x1; p.x1h = a.x1h; p.cq = a.cq; p.M = a.M; p.eps = a.eps;
    p.drop.key = a.drop_key; kzv_drop_params(a.drop_p, &p.drop.thr16, &p.drop.inv_keep);
    kzv_launch_lds<dec_chain_a_kernel>(dim3((a.M + RM - 1) / RM), dim3(512), LDS_A, s, p);
    return kzv_check_launch("dec_chain_a");
}

int kzv_dec_chain_b(const KzvDecChainB& a, hipStream_t s) {
    if (a.M < 1) return kzv_fail(KZV_E_ARG, "dec_chain_b: rows");
    SegB p;
    p.cctx = a.cctx; p.x1 = Resid{a.x1, a.s1, a.st1, a.g1, a.b1}; p.wco = a.wco; p.bco = a.bco; p.g2 = a.g2; p.b2 = a.b2; p.wfc1 = a.wfc1; p.bfc1 = a.bfc1; p.wfc2 = a.wfc2; p.bfc2 = a.bfc2;
    p.g3 = a.g3; p.b3 = a.b3; p.wqkv = a.wqkv; p.bqkv = a.bqkv;
    p.s2 = a.s2; p.st2 = a.st2; p.x2 = a.x2; p.x2h = a.x2h; p.pre = a.pre; p.act = a.act; p.s3 = a.s3; p.st3 = a.st3; p.x3 = a.x3; p.x3h = a.x3h; p.qkv = a.qkv;
    p.M = a.M; p.eps = a.eps;
    p.drop3.key = a.drop3_key; kzv_drop_params(a.drop_p, &p.drop3.thr16, &p.drop3.inv_keep);
    p.drop4.key = a.drop4_key; kzv_drop_params(a.drop_p, &p.drop4.thr16, &p.drop4.inv_keep);
    kzv_launch_lds<dec_chain_b_kernel>(dim3((a.M + RM - 1) / RM), dim3(512), LDS_B, s, p);
    return kzv_check_launch("dec_chain_b");
}
