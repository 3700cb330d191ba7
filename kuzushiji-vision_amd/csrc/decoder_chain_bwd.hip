// The BACKWARD of a decoder layer's linear chains on the row-panel scheme of decoder_chain.hip (dec_rows.h has what the two share):
// dec_lin_kernel, one input-gradient GEMM per launch, and dec_bwd_seg_kernel, a whole row-local segment (GEMM -> LayerNorm backward ->
// GEMM) per launch.
#include "dec_rows.h"
#include "../../include/kzv.h"
#include "kzv_host.h"
#include "kzv_kernels.h"

namespace {

// ---- the decoder's input-gradient GEMMs on the same row-panel scheme (round 4; VERDICT r03 item 5, first half) --------------------
// dX[M, N] = dY[M, K] . W[K-out, N-in] for the six nn.Linear of a RobertaLayer (HF modeling_roberta.py:421-464) and the head's dense
// layer, B operand = the transposed weight copy in fragment order (a second set of packs, refreshed with the first).  At ~15k rows
// each of these was a 16 - 22 us launch of the 128 x 128 kernel at 7 % MFMA utilisation; one workgroup per 64 rows streams the
// weights from L2 through chain_gemm's window and leaves through an LDS tile as whole rows.  Epilogues: bf16 store; fp32 store of
// (acc + residual gradient) -- the "RESID" input-gradient form, residual optional; bf16 store of acc * gelu'(pre-activation) (DGELU).
// The weight gradients stay the grouped gemm_tn launch; the LayerNorm backward between the GEMMs stays its own kernel.
enum { DL_BF16 = 0, DL_RESID = 1, DL_DGELU = 2 };
struct DecLin { const bf16_t* a; const bf16_t* wp; void* out; const float* resid; const bf16_t* aux; int M; };
// the tiles of dec_lin_kernel<CB, KS, EPI>: operand rows of K + 8 bf16, output rows of N + 4 fp32 (RESID) or N + 8 bf16, one after the other in the same memory
template <int CB, int KS> struct DecLinTiles { static constexpr int K = KS * 32, N = CB * 128, LDA = K + 8, LDO16 = N + 8, LDO32 = N + 4; };
template <int CB, int KS, int EPI>
constexpr int dec_lin_lds() {
    using T = DecLinTiles<CB, KS>;
    return RM * lds_max(T::LDA * 2, EPI == DL_RESID ? T::LDO32 * 4 : T::LDO16 * 2);
}
static_assert(dec_lin_lds<2, 8, DL_BF16>() == 33792 && dec_lin_lds<2, 8, DL_RESID>() == 66560 && dec_lin_lds<2, 24, DL_RESID>() == 99328 && dec_lin_lds<6, 8, DL_DGELU>() == 99328,
              "dec_lin: dynamic LDS");
template <int CB, int KS, int EPI>
__global__ __launch_bounds__(512) void dec_lin_kernel(const DecLin p) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    using T = DecLinTiles<CB, KS>;
    constexpr int K = T::K, N = T::N, LDA = T::LDA, LDO16 = T::LDO16, LDO32 = T::LDO32;
    bf16_t* at = (bf16_t*)smem;                                   // [RM][LDA] operand rows; the output tile aliases it after the GEMM
    const int tid = threadIdx.x, lane0 = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int m0 = blockIdx.x * RM;
    bf16x8 R[WIN];
    fill_window<CB, KS, NW, WIN>(R, wave_frags<CB, KS>(p.wp, w), opaque(lane0));
    {
        const int t2 = opaque(tid);
#pragma unroll
        for (int q = 0; q < RM * (K / 8) / 512; ++q) {
            const int idx = t2 + q * 512, row = idx / (K / 8), ch = idx - row * (K / 8);
            uint4 v = make_uint4(0, 0, 0, 0);
            if (m0 + row < p.M) v = *(const uint4*)(p.a + (int64_t)(m0 + row) * K + ch * 8);
            *(uint4*)(at + row * LDA + ch * 8) = v;
        }
    }
    wg_barrier();
    const int lane = opaque(lane0), l15 = lane & 15, g = lane >> 4;
    f32x4 acc[CB][RT];
    chain_gemm<CB, KS, CB, KS, false>(R, wave_frags<CB, KS>(p.wp, w), nullptr, at, LDA, lane, acc);
    wg_barrier();                                                 // every wave has read the operand tile: it becomes the output tile
    if constexpr (EPI == DL_RESID) {
        float* ot = (float*)smem;                                 // [RM][LDO32] fp32
#pragma unroll
        for (int c = 0; c < CB; ++c) {
            const int n0 = (w + 8 * c) * 16 + 4 * g;
#pragma unroll
            for (int rt = 0; rt < RT; ++rt) *(f32x4*)(ot + (rt * 16 + l15) * LDO32 + n0) = acc[c][rt];
        }
        wg_barrier();
        const int t2 = opaque(tid);
#pragma unroll
        for (int q = 0; q < RM * (N / 4) / 512; ++q) {
            const int idx = t2 + q * 512, row = idx / (N / 4), ch = idx - row * (N / 4);
            if (m0 + row < p.M) {
                float4 v = *(const float4*)(ot + row * LDO32 + ch * 4);
                if (p.resid) { const float4 r = *(const float4*)(p.resid + (int64_t)(m0 + row) * N + ch * 4); v.x += r.x; v.y += r.y; v.z += r.z; v.w += r.w; }
                *(float4*)((float*)p.out + (int64_t)(m0 + row) * N + ch * 4) = v;
            }
        }
    } else {
        bf16_t* ot = (bf16_t*)smem;                               // [RM][LDO16] bf16
#pragma unroll
        for (int c = 0; c < CB; ++c) {
            const int n0 = (w + 8 * c) * 16 + 4 * g;
#pragma unroll
            for (int rt = 0; rt < RT; ++rt) {
                f32x4 v = acc[c][rt];
                if constexpr (EPI == DL_DGELU) {                  // the forward's saved gelu'(pre-activation), as nt_emit<KZV_EPI_DGELU>
                    const int m = m0 + rt * 16 + l15;
                    uint2 u = make_uint2(0, 0);
                    if (m < p.M) u = *(const uint2*)(p.aux + (int64_t)m * N + n0);
                    scale_by_bf16x4(v, u);
                }
                *(uint2*)(ot + (rt * 16 + l15) * LDO16 + n0) = make_uint2(pack_bf2(v[0], v[1]), pack_bf2(v[2], v[3]));
            }
        }
        wg_barrier();
        const int t2 = opaque(tid);
#pragma unroll
        for (int q = 0; q < RM * (N / 8) / 512; ++q) {
            const int idx = t2 + q * 512, row = idx / (N / 8), ch = idx - row * (N / 8);
            if (m0 + row < p.M) *(uint4*)((bf16_t*)p.out + (int64_t)(m0 + row) * N + ch * 8) = *(const uint4*)(ot + row * LDO16 + ch * 8);
        }
    }
}

// ---- a decoder layer's BACKWARD linear chains (round 4, VERDICT r03 item 5, second half) ---------------------------------------------
// Between the two attention backwards a RobertaLayer's backward is row-local too (HF modeling_roberta.py:421-464 read upwards):
//   [input gradient of the Linear below a LayerNorm (+ the residual gradient)] -> LayerNorm backward -> [dropout mask, bf16] ->
//   [input gradient of the Linear above it]
// three times per layer (LN3: next layer's qkv | fc2 with gelu';  LN2: fc1 | cross output;  LN1: cross query | self output).  As
// launches these were gemm_nt / dec_lin (12.5 - 20.7 us) + ln_bwd_fast<1> (15.5 us) + gemm_nt / dec_lin (7.4 - 20.7 us); one workgroup
// takes 64 rows through all three with the forward chains' machinery (weights in fragment order through chain_gemm's window, operand
// tiles in LDS, every tensor out as whole rows).  Same arithmetic and rounding points as the launches it replaces: fp32 GEMM result
// + fp32 residual gradient, ln_bwd_fast_kernel's row arithmetic (lane = 4 columns, wave_sum), bf16(mask * dx) as the next operand,
// bf16 output (times the saved gelu' for fc2).  The weight gradients (which read dy16 / out2) stay the grouped gemm_tn launch; gamma /
// beta partial sums go to layernorm.hip's regions (one atomic per column and workgroup).
struct SegBwd {
    const bf16_t* a; const bf16_t* wp1; const float* resid;
    const float* x; const float* st; const float* gamma;
    float* dsum; bf16_t* dy16; Drop odrop; float* partial;
    const bf16_t* wp2; const bf16_t* aux; bf16_t* out2; int M;
};
// the tiles of dec_bwd_seg_kernel<KS1, NP2>: the 256-wide operand tile of GEMM 2, then ONE region that is in turn GEMM 1's operand rows
// (K1 + 8 bf16), the fp32 d tile (LDS_ floats) and GEMM 2's output rows (N2 + 8 bf16)
template <int KS1, int NP2> struct SegTiles { static constexpr int K1 = KS1 * 32, LDA = K1 + 8, N2 = NP2 * 256, LDO = N2 + 8; };
template <int KS1, int NP2>
constexpr int dec_bwd_seg_lds() {
    using T = SegTiles<KS1, NP2>;
    return LDS_A1 + RM * lds_max(lds_max(T::LDA * 2, T::LDO * 2), LDS_ * 4);
}
static_assert(dec_bwd_seg_lds<8, 1>() == 100352 && dec_bwd_seg_lds<24, 1>() == 133120 && dec_bwd_seg_lds<8, 3>() == 133120 && dec_bwd_seg_lds<24, 3>() == 133120,
              "dec_bwd_seg: dynamic LDS");
template <int KS1, int NP2>
__global__ __launch_bounds__(512) void dec_bwd_seg_kernel(const SegBwd p) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    using T = SegTiles<KS1, NP2>;
    constexpr int K1 = T::K1, LDA = T::LDA, N2 = T::N2, LDO = T::LDO;
    bf16_t* a1 = (bf16_t*)smem;                                   // [RM][LDH] bf16(mask * dx): GEMM 2's operand
    char* xr = smem + LDS_A1;                                     // GEMM 1's operand rows -> the fp32 d tile -> partial sums -> GEMM 2's output rows
    bf16_t* at = (bf16_t*)xr; float* t32 = (float*)xr; bf16_t* ot = (bf16_t*)xr;
    const int tid = threadIdx.x, lane0 = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int m0 = blockIdx.x * RM;
    bf16x8 R[WIN];
    SEG_STAMP(16);
    fill_window<2, KS1, NW, WIN>(R, wave_frags<2, KS1>(p.wp1, w), opaque(lane0));
    {
        const int t2 = opaque(tid);
#pragma unroll
        for (int q = 0; q < RM * (K1 / 8) / 512; ++q) {
            const int idx = t2 + q * 512, row = idx / (K1 / 8), ch = idx - row * (K1 / 8);
            uint4 v = make_uint4(0, 0, 0, 0);
            if (m0 + row < p.M) v = *(const uint4*)(p.a + (int64_t)(m0 + row) * K1 + ch * 8);
            *(uint4*)(at + row * LDA + ch * 8) = v;
        }
    }
    // the LayerNorm backward's global operands of this wave's eight rows, requested now: they arrive under GEMM 1 (rows past M: the last row)
    float4 xv8[RM / 8], rv8[RM / 8]; float2 st8[RM / 8];
    {
        const int lane = opaque(lane0);
#pragma unroll
        for (int q = 0; q < RM / 8; ++q) {
            const int64_t mc = min(m0 + w * (RM / 8) + q, p.M - 1);
            xv8[q] = *(const float4*)(p.x + mc * HD + lane * 4);
            rv8[q] = *(const float4*)((p.resid ? p.resid : p.x) + mc * HD + lane * 4);      // no branch around a load (unused without a residual)
            st8[q] = *(const float2*)(p.st + 2 * mc);
        }
    }
    wg_barrier();
    SEG_STAMP(17);
    {
        const int lane = opaque(lane0), l15 = lane & 15, g = lane >> 4;
        f32x4 acc[2][RT];
        chain_gemm<2, KS1, 2, 8, true>(R, wave_frags<2, KS1>(p.wp1, w), wave_frags<2, 8>(p.wp2, w), at, LDA, lane, acc);
        wg_barrier();                                             // every wave has read the operand rows: the fp32 tile takes their place
        SEG_STAMP(18);
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            const int n0 = (w + 8 * c) * 16 + 4 * g;
#pragma unroll
            for (int rt = 0; rt < RT; ++rt) *(f32x4*)(t32 + (rt * 16 + l15) * LDS_ + n0) = acc[c][rt];
        }
    }
    wg_barrier();
    SEG_STAMP(19);
    float4 dg = make_float4(0, 0, 0, 0), db = make_float4(0, 0, 0, 0);
    {   // LayerNorm backward, wave w: rows 8 w .. 8 w + 7 (ln_bwd_fast_kernel<1, true, false>'s arithmetic: kzv_common.h ln_bwd_*)
        const int lane = opaque(lane0);
        const float4 gm = *(const float4*)(p.gamma + lane * 4);
        const float invH = 1.f / (float)HD;
        retire_loads();                                           // the operands requested before GEMM 1: retired by hand (see pin)
#pragma unroll
        for (int q = 0; q < RM / 8; ++q) { pin(xv8[q]); pin(rv8[q]); pin(st8[q]); }
        float4 d8[RM / 8];                                        // every row out of LDS before the first LDS store below (hipcc keeps their order otherwise: one row at a time)
#pragma unroll
        for (int q = 0; q < RM / 8; ++q) d8[q] = *(const float4*)(t32 + (w * (RM / 8) + q) * LDS_ + lane * 4);
        // per row ln_bwd_fast_kernel's statements (kzv_common.h ln_bwd_*; the rows' wave sums one after the other, as there)
#pragma unroll
        for (int q = 0; q < RM / 8; ++q) {
            const int row = w * (RM / 8) + q, m = m0 + row;
            if (m >= p.M) {                                       // wave-uniform
                *(uint2*)(a1 + row * LDH + lane * 4) = make_uint2(0, 0);
                continue;
            }
            float4 d = d8[q];
            if (p.resid) { const float4 r = rv8[q]; d.x += r.x; d.y += r.y; d.z += r.z; d.w += r.w; }
            const float rstd = st8[q].y;
            const LnBwdTerms t = ln_bwd_terms(d, xv8[q], gm, st8[q].x, rstd);
            const float s1 = __fadd_rn(0.f, t.s1), s2 = __fadd_rn(0.f, t.s2);
            ln_bwd_accum(dg, db, d, t);
            const float m1 = __fmul_rn(wave_sum(s1), invH), m2 = __fmul_rn(wave_sum(s2), invH);
            float4 o = ln_bwd_dx(t, m1, m2, rstd);
            *(float4*)(p.dsum + (int64_t)m * HD + lane * 4) = o;
            if (p.odrop.thr16) KZV_DROP4(o.x, o.y, o.z, o.w, p.odrop.key, (unsigned)m * (unsigned)HD + 4u * lane, p.odrop.thr16, p.odrop.inv_keep);
            const uint2 h = make_uint2(pack_bf2(o.x, o.y), pack_bf2(o.z, o.w));
            *(uint2*)(p.dy16 + (int64_t)m * HD + lane * 4) = h;
            *(uint2*)(a1 + row * LDH + lane * 4) = h;
        }
    }
    SEG_STAMP(20);
    wg_barrier();                                                 // the fp32 tile is dead: it holds the eight waves' gamma / beta partial sums
    {
        const int lane = opaque(lane0);
        float4* sg = (float4*)xr + (w * 2) * 64;
        sg[lane] = dg; sg[64 + lane] = db;
    }
    wg_barrier();
    {
        const int t2 = opaque(tid), col = t2 & 255, which = t2 >> 8;
        const float* sf = (const float*)xr;
        float a = 0.f;
#pragma unroll
        for (int ww = 0; ww < 8; ++ww) a += sf[(ww * 2 + which) * HD + col];
        atomicAdd(p.partial + (size_t)(blockIdx.x % KZV_LN_SLOTS) * 2 * HD + which * HD + col, a);
    }
    wg_barrier();                                                 // ... and now GEMM 2's output rows
    SEG_STAMP(21);
    {
        const int lane = opaque(lane0), l15 = lane & 15, g = lane >> 4;
#pragma unroll
        for (int pass = 0; pass < NP2; ++pass) {
            uint2 u[2][RT];
            if constexpr (NP2 > 1) {                              // fc2: the forward's saved gelu'(pre-activation), requested before the MFMAs
#pragma unroll
                for (int c = 0; c < 2; ++c)
#pragma unroll
                    for (int rt = 0; rt < RT; ++rt) {
                        const int64_t m = min(m0 + rt * 16 + l15, p.M - 1);     // rows past M: the last row's (their products are never stored)
                        u[c][rt] = *(const uint2*)(p.aux + m * N2 + 256 * pass + (w + 8 * c) * 16 + 4 * g);
                    }
            }
            f32x4 acc[2][RT];
            if (pass + 1 < NP2) chain_gemm<2, 8, 2, 8, true>(R, wave_frags<2, 8>(p.wp2 + (int64_t)pass * 65536, w), wave_frags<2, 8>(p.wp2 + (int64_t)(pass + 1) * 65536, w), a1, LDH, lane, acc);
            else chain_gemm<2, 8, 2, 8, false>(R, wave_frags<2, 8>(p.wp2 + (int64_t)pass * 65536, w), nullptr, a1, LDH, lane, acc);
            if constexpr (NP2 > 1) {                              // gelu' (requested before the MFMAs): retired by hand
                retire_loads();
#pragma unroll
                for (int c = 0; c < 2; ++c)
#pragma unroll
                    for (int rt = 0; rt < RT; ++rt) pin(u[c][rt]);
            }
#pragma unroll
            for (int c = 0; c < 2; ++c) {
                const int n0 = 256 * pass + (w + 8 * c) * 16 + 4 * g;
#pragma unroll
                for (int rt = 0; rt < RT; ++rt) {
                    f32x4 v = acc[c][rt];
                    if constexpr (NP2 > 1) scale_by_bf16x4(v, u[c][rt]);
                    *(uint2*)(ot + (rt * 16 + l15) * LDO + n0) = make_uint2(pack_bf2(v[0], v[1]), pack_bf2(v[2], v[3]));
                }
            }
        }
    }
    SEG_STAMP(22);
    wg_barrier();
    rows_out<32 * NP2>(ot, LDO, p.out2, N2, m0, p.M, opaque(tid));
    SEG_STAMP(23);
}

}  // namespace

#ifdef KZV_STAMPS      // this unit's stamp array (dec_bwd_seg writes slots 16 - 23): tools/dev/stamps_seg.py
extern "C" int kzv_debug_seg_stamps(long long* host, int n) {
    return hipMemcpyFromSymbol(host, HIP_SYMBOL(g_chain_stamps), sizeof(long long) * (n < 32 ? n : 32)) == hipSuccess ? 0 : 1;
}
#endif

// N / K: output / reduction width (256 or 768, not both 768); epi: 0 bf16, 1 fp32 (+ resid), 2 bf16 * aux
int kzv_dec_lin(const bf16_t* a, const bf16_t* wp, void* out, const float* resid, const bf16_t* aux, int M, int N, int K, int epi, hipStream_t s) {
    if (!a || !wp || !out || M < 1 || (epi == DL_DGELU && !aux)) return kzv_fail(KZV_E_ARG, "dec_lin: bad argument");
    DecLin p{a, wp, out, resid, aux, M};
    const dim3 grid((M + RM - 1) / RM);
#define KZV_DL(CB_, KS_, E_) do { kzv_launch_lds<dec_lin_kernel<CB_, KS_, E_>>(grid, dim3(512), dec_lin_lds<CB_, KS_, E_>(), s, p); return kzv_check_launch("dec_lin"); } while (0)
    if (N == 256 && K == 256 && epi == DL_BF16) KZV_DL(2, 8, DL_BF16);
    if (N == 256 && K == 256 && epi == DL_RESID) KZV_DL(2, 8, DL_RESID);
    if (N == 256 && K == 768 && epi == DL_RESID) KZV_DL(2, 24, DL_RESID);
    if (N == 768 && K == 256 && epi == DL_DGELU) KZV_DL(6, 8, DL_DGELU);
#undef KZV_DL
    return kzv_fail(KZV_E_ARG, "dec_lin: no instance for N %d, K %d, epilogue %d", N, K, epi);
}

int kzv_dec_bwd_seg(const KzvDecBwdSeg& a, hipStream_t s) {
    if (!a.a || !a.wp1 || !a.x || !a.st || !a.gamma || !a.dgamma || !a.dbeta || !a.dsum || !a.dy16 || !a.wp2 || !a.out2 || a.M < 1 || (a.K1 != 256 && a.K1 != 768))
        return kzv_fail(KZV_E_ARG, "dec_bwd_seg: bad argument");
    bool fold_now = false;
    float* partial = kzv_ln_partial_region(a.dgamma, a.dbeta, HD, s, &fold_now);
    if (!partial) return KZV_E_ARG;
    SegBwd p{a.a, a.wp1, a.resid, a.x, a.st, a.gamma, a.dsum, a.dy16, Drop{0, 1.f, a.drop_key}, partial, a.wp2, a.aux, a.out2, a.M};
    kzv_drop_params(a.drop_p, &p.odrop.thr16, &p.odrop.inv_keep);
    const dim3 grid((a.M + RM - 1) / RM);
#define KZV_SEG(KS1_, NP2_) kzv_launch_lds<dec_bwd_seg_kernel<KS1_, NP2_>>(grid, dim3(512), dec_bwd_seg_lds<KS1_, NP2_>(), s, p)
    if (a.K1 == 256 && !a.aux) KZV_SEG(8, 1);
    else if (a.K1 == 768 && !a.aux) KZV_SEG(24, 1);
    else if (a.K1 == 256) KZV_SEG(8, 3);
    else KZV_SEG(24, 3);
#undef KZV_SEG
    { const int rc = kzv_check_launch("dec_bwd_seg"); if (rc != KZV_OK) return rc; }
    return fold_now ? kzv_ln_partial_fold(partial, a.dgamma, a.dbeta, HD, s) : KZV_OK;
}
