// N1: the KV-cached generation step of the whole decoder in ONE launch.
//
// Replaces, per new token, the embedding gather + 6 x (QKV, cached self-attention, output projection, cross query, cross-attention,
// output projection, fc1 + GELU, fc2) + the LM head's dense layer of HF RobertaForCausalLM with `use_cache=True`
// (modeling_roberta.py:75-122, 186-326, 421-464, 877-893 as driven by src/models/trocr_model.py:306-316, num_beams = 4): 50 launches
// of 5-15 us became one.
//
// Every operation of a decoder step is local to a sequence -- the linears are row-wise, a sequence attends to its own cache and to
// its own image's patch keys -- so ONE workgroup owns the G sequences of one image (G = beams) through all layers and never talks
// to another workgroup: no grid barrier, no flags.  Hidden size 256, 4 heads of 64, FFN 768 (the reference decoder), <= 128 cached
// keys, <= 320 patch keys (one cross-attention path, cross_chunk_*: up to 160 keys are its NC = 1 instance, one pass through the
// attention waves' registers; 161 .. 320 go through them in NC chunks with an online softmax); other geometries keep the
// launch-per-operation path (model.cpp).
//
// What bounds it is ONE CU's load path (~60 GB/s from L2): per token a workgroup streams all 9.4 MB of decoder weights plus its
// sequences' attention rows.  So the eight waves are split by what they LOAD, and each stream stays in flight across the barriers:
//   * waves 0-3, the linears: the 16-row MFMA tile holds the G rows (lanes of rows >= G repeat row G - 1); wave w owns the
//     16-column blocks w, w + 4, ... and reads its weight fragments in MFMA fragment order (frag_stream.h: a wave-instruction is one
//     contiguous KiB), a window of 16 fragments always in flight and refilled with the NEXT linear's first fragments as a linear ends.
//   * waves 4-7, attention, one head each: key / value rows go to registers (a wave-instruction = 8 rows x 128 B) and are requested
//     one phase early -- the cached rows of the first sequence while the QKV projection runs, the image's patch keys / values
//     (shared by the beams) while the output projection, LayerNorm and cross query run -- so the HBM latency of one stream hides
//     behind the L2 stream of the other; between the two they also fetch the next layer's biases and LayerNorm weights into LDS.
//   * a vector-memory counter retires in issue order, which is why the two kinds of load cannot share a wave: a weight fragment
//     issued behind an HBM row would wait for it.
#include "kzv_common.h"
#include "../../include/kzv.h"
#include "kzv_host.h"
#include "kzv_kernels.h"
#include "frag_stream.h"
#include <cmath>

namespace {

constexpr int HD = 256, NH = 4, FD = 768, TMAX = 128, NPMAX = 160;
constexpr int LDX = HD + 4;          // fp32 rows of the residual stream in LDS
constexpr int LDH = HD + 8;          // bf16 rows, 256 wide (16-byte aligned, 4 banks apart)
constexpr int LDW = FD + 8;          // bf16 rows, 768 wide (qkv / FFN activation)
// one layer's biases and LayerNorm weights in LDS (floats)
constexpr int PB_QKV = 0, PB_O = 768, PB_CQ = 1024, PB_CO = 1280, PB_FC1 = 1536, PB_FC2 = 2304;
constexpr int PL1W = 2560, PL1B = 2816, PL2W = 3072, PL2B = 3328, PL3W = 3584, PL3B = 3840, PAR = 4096;
constexpr int NR = 40;               // role registers: 40 fragments (160 VGPRs): the weight window, or key + value rows
constexpr int NLW = 4, WIN = 24;     // the linear waves, and the bf16 weight fragments each keeps in flight (frag_stream.h)
constexpr int NIS = TMAX / 8, NIC = NPMAX / 8;
constexpr int NPWIDE = 320, NIW = NPWIDE / 8;      // the chunked instances: 161 .. 320 patch keys, NIW key iterations in all
#ifndef KZV_DF_CHUNKS
#define KZV_DF_CHUNKS 2                            // chunks of the 320 keys (2, 4 or 8): DESIGN.md section 7, N1 has the measurements
#endif

// Sums / maxima over lane groups without the LDS crossbar (ds_bpermute, what __shfl_xor compiles to): DPP moves for the steps inside a
// 16-lane row, the crossbar only for the two steps across rows.
template <int CTRL> __device__ __forceinline__ float dpp_mov(float v) {
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xf, 0xf, false));
}
// sum over the 8 lanes of a key row: quad_perm [1,0,3,2], quad_perm [2,3,0,1], row_half_mirror (the other quad's sum)
__device__ __forceinline__ float sum8(float a) { a += dpp_mov<0xB1>(a); a += dpp_mov<0x4E>(a); a += dpp_mov<0x141>(a); return a; }
// sum over the 8 key rows of a wave-instruction (lanes with equal lane & 7): row_ror:8, then the two cross-row steps
__device__ __forceinline__ float sum_rows(float a) { a += dpp_mov<0x128>(a); a += __shfl_xor(a, 16, 64); a += __shfl_xor(a, 32, 64); return a; }
__device__ __forceinline__ float wave_sum_d(float a) { return sum_rows(sum8(a)); }
__device__ __forceinline__ float wave_max_d(float a) {
    a = fmaxf(a, dpp_mov<0xB1>(a)); a = fmaxf(a, dpp_mov<0x4E>(a)); a = fmaxf(a, dpp_mov<0x141>(a)); a = fmaxf(a, dpp_mov<0x128>(a));
    a = fmaxf(a, __shfl_xor(a, 16, 64)); a = fmaxf(a, __shfl_xor(a, 32, 64));
    return a;
}

// q . k over this lane's 8 dimensions in fp32 (products of bf16 pairs are exact, eight fp32 accumulations); qp = the query pre-scaled
// by 1 / 8 (exact in bf16), two dimensions per dword.  NOT v_dot2c_f32_bf16: four of those per key are 4x fewer instructions, and
// moved the step's logits 4 - 6x further from the teacher-forced recompute (3e-2 against 5e-3 twelve layers deep,
// tests/test_decode_fused_gpu.py) -- its accumulation is not an fp32 FMA chain.
typedef __attribute__((ext_vector_type(4))) unsigned u32x4_t;
__device__ __forceinline__ float dot8(const bf16x8& k, const u32x4_t& qp) {
    const u32x4_t kd = __builtin_bit_cast(u32x4_t, k);
    float a = 0.f;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        a += __builtin_bit_cast(float, kd[e] << 16) * __builtin_bit_cast(float, qp[e] << 16);
        a += __builtin_bit_cast(float, kd[e] & 0xffff0000u) * __builtin_bit_cast(float, qp[e] & 0xffff0000u);
    }
    return a;
}
__device__ __forceinline__ u32x4_t scaled_query(const bf16_t* q) {
    const bf16x8 q8 = *(const bf16x8*)q;
    return (u32x4_t){pack_bf2(bf2f((bf16_t)q8[0]) * 0.125f, bf2f((bf16_t)q8[1]) * 0.125f), pack_bf2(bf2f((bf16_t)q8[2]) * 0.125f, bf2f((bf16_t)q8[3]) * 0.125f),
                     pack_bf2(bf2f((bf16_t)q8[4]) * 0.125f, bf2f((bf16_t)q8[5]) * 0.125f), pack_bf2(bf2f((bf16_t)q8[6]) * 0.125f, bf2f((bf16_t)q8[7]) * 0.125f)};
}

#ifdef KZV_STAMPS      // diagnostic build (tools/dev/stamps_decode.py): the phase timeline of workgroup 0, layer 0 and the last layer
__device__ long long g_df_stamps[64];
#define DF_STAMP(k) do { if (blockIdx.x == 0 && threadIdx.x == 0) g_df_stamps[k] = (long long)__builtin_amdgcn_s_memtime(); } while (0)
#define DF_STAMP_L(k) do { if (li == 0) DF_STAMP(2 + (k)); else if (li == p.nlayers - 1) DF_STAMP(20 + (k)); } while (0)
#define DF_STAMP_A(k) do { if (blockIdx.x == 0 && threadIdx.x == 256 && li == 1) g_df_stamps[44 + (k)] = (long long)__builtin_amdgcn_s_memtime(); } while (0)
#else
#define DF_STAMP_A(k)
#define DF_STAMP(k)
#define DF_STAMP_L(k)
#endif

template <int G>
struct Lds {
    float xs[G][LDX];                // x = LN(s): the residual stream (fp32)
    float ss[G][LDX];                // a sub-layer's output before its LayerNorm
    bf16_t ab[G][LDH];               // x as the next GEMM's A operand
    bf16_t wide[G][LDW];             // q | k | v of this step, then the cross query, then the FFN activation
    bf16_t ctx[G][LDH];              // attention output
    float par[2][PAR];               // biases + LayerNorm weights of this layer / the next one
    int rt[G][TMAX];                 // beam row table of the G sequences (cache row of the ancestor that wrote key j)
    unsigned char vf[G][TMAX];       // usable-key flags
};

// ---- the weight stream (waves 0-3) --------------------------------------------------------------------------------------------
// acc[c][r] = sum_k W[n][k] * a[m][k] for m = lane & 15 (rows >= G repeat row G - 1), n = (w + 4 c) * 16 + 4 (lane >> 4) + r.
// The fragment order of Wp, the window and its refill rule: frag_stream.h.
template <int CB, int KS, int NCB, int NKS, int OFF, int G>      // OFF: window slot of this GEMM's fragment 0 (the stream's fragments take the slots in turn)
__device__ __forceinline__ void rows_gemm(bf16x8 (&R)[NR], const char* wb, const char* next, const bf16_t* a_lds, int lda, int lane, f32x4 (&acc)[CB]) {
    constexpr int F = CB * KS;
    static_assert(F >= WIN && NCB * NKS >= WIN && WIN <= NR, "rows_gemm: window");
    const int l15 = lane & 15, g = lane >> 4;
    const unsigned wo = (unsigned)lane * 16u;
    const bf16_t* ap = a_lds + min(l15, G - 1) * lda + g * 8;
#pragma unroll
    for (int c = 0; c < CB; ++c) acc[c] = (f32x4){0.f, 0.f, 0.f, 0.f};
    bf16x8 fa;
#pragma unroll
    for (int i = 0; i < F; ++i) {
        const int ks = i / CB, c = i % CB, slot = (OFF + i) % WIN;
        if (c == 0) fa = *(const bf16x8*)(ap + ks * 32);
        acc[c] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(R[slot], fa, acc[c], 0, 0, 0);
        if (i + WIN < F) R[slot] = ld_frag<CB, KS, NLW>(wb, wo, i + WIN);
        else if (next) R[slot] = ld_frag<NCB, NKS, NLW>(next, wo, i + WIN - F);
    }
}

// ---- the same stream as OCP e4m3 (kzv_set_decode_weights) -------------------------------------------------------------------------
// Half the bytes per weight, the same 96 KiB in flight: a window slot is a 64-DEEP fragment -- the lane's 8 bytes of k-step 2 j, then
// its 8 bytes of k-step 2 j + 1 -- and wave w's fragments of ALL linears lie in the order it consumes them, as one contiguous stream
// (quant_pack8_kernel): per layer QKV half 0 | half 1 | O | CQ | CO | FC1 half 0 | half 1 | FC2 (S8_LAYER fragments), then the head's
// dense layer, then WIN8 fragments of zeros.  So a refill is `slot = stream[position + WIN8]`, whatever GEMM that position belongs to:
// no pointer to a next GEMM, no condition, and no load past the allocation.  Widened to bf16 in registers (both conversions exact),
// a fragment feeds the same two MFMAs in the same order as rows_gemm's, so with W = q * 2^e per output row the accumulators are
// 2^-e times the bf16 step's, bit for bit, and the epilogue's acc * 2^e + bias restores them.
#ifndef KZV_DF_WIN8
#define KZV_DF_WIN8 24                             // e4m3 fragments (1 KiB per wave each) in flight per linear wave; 32 also builds spill-free: DESIGN.md section 7, N1 has both timed
#endif
constexpr int WIN8 = KZV_DF_WIN8;                  // the e4m3 stream's window only: the bf16 stream keeps WIN
constexpr int S8_QKV = 0, S8_O = 48, S8_CQ = 64, S8_CO = 80, S8_FC1 = 96, S8_FC2 = 144, S8_LAYER = 192, S8_HEAD = 16;
constexpr int SCL = 2560;            // a layer's row scales in LDS, in the order of its biases (PB_*); the head's take [0, 256)
static_assert(S8_LAYER % WIN8 == 0, "a layer's e4m3 fragments must fill the window a whole number of times");
__device__ __forceinline__ bf16x8 widen8(unsigned lo, unsigned hi) {
    // v_cvt_pk_f32_fp8 (the low, then the high byte pair of a dword), v_cvt_pk_bf16_f32: 8 conversions per 8 weights
    const f2_t a = __builtin_amdgcn_cvt_pk_f32_fp8((int)lo, false), b = __builtin_amdgcn_cvt_pk_f32_fp8((int)lo, true);
    const f2_t c = __builtin_amdgcn_cvt_pk_f32_fp8((int)hi, false), d = __builtin_amdgcn_cvt_pk_f32_fp8((int)hi, true);
    const u32x4_t r = {pack_bf2(a[0], a[1]), pack_bf2(b[0], b[1]), pack_bf2(c[0], c[1]), pack_bf2(d[0], d[1])};
    return __builtin_bit_cast(bf16x8, r);
}
__device__ __forceinline__ void fill_window8(bf16x8 (&R)[NR], const char* sb, int lane) {
    const unsigned wo = (unsigned)lane * 16u;
#pragma unroll
    for (int i = 0; i < WIN8; ++i) R[i] = *(const bf16x8*)(sb + i * 1024 + wo);
}
// sb = the wave's stream at this layer's first fragment; POS = this GEMM's first fragment in the layer (and, mod WIN8, its window slot);
// KS counts 32-deep k-steps as rows_gemm's does
template <int CB, int KS, int POS, int G>
__device__ __forceinline__ void rows_gemm8(bf16x8 (&R)[NR], const char* sb, const bf16_t* a_lds, int lda, int lane, f32x4 (&acc)[CB]) {
    constexpr int F = CB * KS / 2;
    static_assert(KS % 2 == 0 && WIN8 <= NR, "rows_gemm8: window");
    const int l15 = lane & 15, g = lane >> 4;
    const unsigned wo = (unsigned)lane * 16u;
    const bf16_t* ap = a_lds + min(l15, G - 1) * lda + g * 8;
#pragma unroll
    for (int c = 0; c < CB; ++c) acc[c] = (f32x4){0.f, 0.f, 0.f, 0.f};
    bf16x8 fa0, fa1;
#pragma unroll
    for (int i = 0; i < F; ++i) {
        const int ks2 = i / CB, c = i % CB, slot = (POS + i) % WIN8;
        if (c == 0) { fa0 = *(const bf16x8*)(ap + ks2 * 64); fa1 = *(const bf16x8*)(ap + ks2 * 64 + 32); }
        const u32x4_t q = __builtin_bit_cast(u32x4_t, R[slot]);
        acc[c] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(widen8(q[0], q[1]), fa0, acc[c], 0, 0, 0);
        acc[c] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(widen8(q[2], q[3]), fa1, acc[c], 0, 0, 0);
        R[slot] = *(const bf16x8*)(sb + (POS + i + WIN8) * 1024 + wo);
        __builtin_amdgcn_sched_barrier(0);      // the refill stays behind ITS MFMAs: left to itself hipcc gathers a GEMM's refills at its end and the window drains
    }
}
// the epilogues' "accumulator + bias": with row scales, accumulator * scale + bias (a power of two: fused or not, the same bits)
template <bool F8> __device__ __forceinline__ float4 scale4(const float* scl, int at) {
    if constexpr (F8) return *(const float4*)(scl + at);
    else return make_float4(1.f, 1.f, 1.f, 1.f);
}
template <bool F8> __device__ __forceinline__ float sb_add(float acc, float s, float b) {
    if constexpr (F8) return fmaf(acc, s, b);
    else return acc + b;
}

// ---- quantise-and-pack: bf16 [N, K] -> OCP e4m3 with one power-of-two scale per output row, one launch over a table of matrices ------
// Per row: s = 2^e, the smallest power of two with amax / s <= 448 (the exponent from amax's bits: 448 = 1.75 * 2^8, so e is amax's
// exponent - 8, or - 7 where its fraction exceeds 1.75), clamped to the normal range; an all-zero row keeps s = 1; q = e4m3(w / s),
// round-to-nearest-even (pack_fp8x4).  q * s is a bf16 number: 3 mantissa bits.  One wave per row, 4 weights per lane and pass.
// cb == 0: the bytes stay row-major [N, K] (the per-op entry).  cb = 4 or 6: the decode stream of rows_gemm8 -- 16-row block nb belongs
// to wave nb % 4 as its column block nb / 4 = half * cb + c, and its 64-deep fragment ks2 is fragment pos + half * F + ks2 * cb + c
// of that wave's stream (F = cb * K / 64 fragments per half).
struct Quant8Desc { const bf16_t* src; int N, K, row0, scale_at, cb, pos; };
constexpr int Q8_MAX_JOBS = 8 * KZV_DECODE_FUSED_MAX_LAYERS + 1;       // 32-byte descriptors in the kernel argument block (4 KiB limit)
struct Quant8Table { Quant8Desc d[Q8_MAX_JOBS]; int n, rows, pad_pos; unsigned char* dst; float* scales; int64_t wave_bytes; };
__global__ __launch_bounds__(256) void quant_pack8_kernel(const Quant8Table tab) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= tab.rows) {       // the blocks behind the last row: the WIN8 zero fragments that end each wave's stream
        const int t = (blockIdx.x - tab.rows / 4) * 256 + threadIdx.x;
        if (tab.pad_pos >= 0 && t < 4 * WIN8 * 64)
            *(uint4*)(tab.dst + (int64_t)(t / (WIN8 * 64)) * tab.wave_bytes + ((int64_t)tab.pad_pos * 64 + t % (WIN8 * 64)) * 16) = make_uint4(0, 0, 0, 0);
        return;
    }
    int lo = 0, hi = tab.n - 1;                  // the last job with row0 <= row
    while (lo < hi) { const int mid = (lo + hi + 1) >> 1; if (tab.d[mid].row0 <= row) lo = mid; else hi = mid - 1; }
    const Quant8Desc& d = tab.d[lo];
    const int n = row - d.row0, K = d.K;
    const bf16_t* src = d.src + (int64_t)n * K;
    float amax = 0.f;
    for (int k = lane * 4; k < K; k += 256) {
        const uint2 v = *(const uint2*)(src + k);
        amax = fmaxf(fmaxf(amax, fmaxf(fabsf(bf2f((bf16_t)(v.x & 0xffffu))), fabsf(bf2f((bf16_t)(v.x >> 16))))),
                     fmaxf(fabsf(bf2f((bf16_t)(v.y & 0xffffu))), fabsf(bf2f((bf16_t)(v.y >> 16)))));
    }
    amax = wave_max(amax);
    const unsigned ab = __builtin_bit_cast(unsigned, amax);
    int e = (int)(ab >> 23) - 127 - ((ab & 0x7fffffu) > 0x600000u ? 7 : 8);
    e = amax == 0.f ? 0 : min(max(e, -126), 126);
    const float s = __builtin_bit_cast(float, (unsigned)(e + 127) << 23), inv = __builtin_bit_cast(float, (unsigned)(127 - e) << 23);
    if (lane == 0) tab.scales[d.scale_at + n] = s;
    const int nb = n >> 4, cbg = nb >> 2, cb = d.cb;
    const int64_t frag0 = cb ? (int64_t)d.pos + (cbg / cb) * (cb * (K >> 6)) + cbg % cb : 0;
    unsigned char* out = cb ? tab.dst + (int64_t)(nb & 3) * tab.wave_bytes + (n & 15) * 16 : tab.dst + (int64_t)d.pos + (int64_t)n * K;
    for (int k = lane * 4; k < K; k += 256) {
        const uint2 v = *(const uint2*)(src + k);
        const unsigned q = pack_fp8x4(bf2f((bf16_t)(v.x & 0xffffu)) * inv, bf2f((bf16_t)(v.x >> 16)) * inv, bf2f((bf16_t)(v.y & 0xffffu)) * inv, bf2f((bf16_t)(v.y >> 16)) * inv);
        // in a fragment: lane (n & 15) + 16 * ((k & 31) / 8), byte 8 * ((k & 63) / 32) + (k & 7)
        if (cb) *(unsigned*)(out + (frag0 + (int64_t)(k >> 6) * cb) * 1024 + ((k & 31) >> 3) * 256 + ((k & 63) >> 5) * 8 + (k & 7)) = q;
        else *(unsigned*)(out + k) = q;
    }
}

// LayerNorm of one row (fp32, LDS) by one wave: the normalised row goes to xs (fp32) and ab (bf16); gamma / beta from LDS
__device__ __forceinline__ void ln_row(const float* src, const float* gamma, const float* beta, float eps, float* xs, bf16_t* ab, int lane) {
    const float4 v = *(const float4*)(src + lane * 4);
    const float mean = wave_sum(v.x + v.y + v.z + v.w) * (1.f / HD);
    const float a = v.x - mean, b = v.y - mean, c = v.z - mean, d = v.w - mean;
    const float rstd = rsqrtf(wave_sum(a * a + b * b + c * c + d * d) * (1.f / HD) + eps);
    const float4 ga = *(const float4*)(gamma + lane * 4), be = *(const float4*)(beta + lane * 4);
    const float y0 = a * rstd * ga.x + be.x, y1 = b * rstd * ga.y + be.y, y2 = c * rstd * ga.z + be.z, y3 = d * rstd * ga.w + be.w;
    *(float4*)(xs + lane * 4) = make_float4(y0, y1, y2, y3);
    *(uint2*)(ab + lane * 4) = make_uint2(pack_bf2(y0, y1), pack_bf2(y2, y3));
}

struct FusedLayer {
    const bf16_t *wqkv, *wo, *wcq, *wco, *wfc1, *wfc2;
    const float *bqkv, *bo, *bcq, *bco, *bfc1, *bfc2;
    const float *ln1w, *ln1b, *ln2w, *ln2b, *ln3w, *ln3b;
};
struct FusedP {
    FusedLayer L[KZV_DECODE_FUSED_MAX_LAYERS];
    int nlayers;
    const int64_t* tokens; const int* posids;
    const float *word, *type0, *postab, *elnw, *elnb;
    const bf16_t* whd; const float* bhd; float* hd_out;         // LM head dense + GELU -> fp32 [B, 256]
    bf16_t* cache; int64_t plane;                               // self-attention K / V planes [2 * layer (+1)][B][head][T][64]
    const bf16_t* ckv; int64_t plane2;                          // cross K / V planes [2 * layer (+1)][image][head][npa][64]
    const unsigned char* valid; int64_t ldvalid;
    const int* tptr; int t, T, npa, B;
    int* rows;                                                  // beam row table [B][T] or null
    float eps;
};
struct FusedP8 : FusedP {                                       // the e4m3 instances' arguments (the bf16 instances keep FusedP as it was)
    const char* w8; int64_t wave8;                              // the four waves' fragment streams, wave8 bytes each
    const float* sc8;                                           // row scales [layer][SCL], then the head's 256
};
// the slot instances' arguments (slot-refill decoding, kzv_stream_*): workgroup b serves image slot_image[b] (< 0: idle) at ITS step
// slot_t[b]; both derive, so every other instance keeps its argument layout
struct FusedPS : FusedP { const int* slot_image; const int* slot_t; };
struct FusedPS8 : FusedP8 { const int* slot_image; const int* slot_t; };
template <bool F8, bool SL = false> struct FusedArgs { typedef FusedP type; };
template <> struct FusedArgs<true, false> { typedef FusedP8 type; };
template <> struct FusedArgs<false, true> { typedef FusedPS type; };
template <> struct FusedArgs<true, true> { typedef FusedPS8 type; };

// ---- the attention streams (waves 4-7, head h each) ------------------------------------------------------------------------------
// lane = (row r = lane >> 3 of an 8-key group, 16-byte piece c = lane & 7); iteration i holds key 8 i + r.
// cached keys -> R[0 .. NIS), values -> R[NIS .. 2 NIS) for sequence g.  Every load is unconditional and clamped to a written
// position: this step's own key / value comes from LDS and positions past it are dropped in self_compute.
template <int G, bool KEYS, bool VALUES>
__device__ __forceinline__ void self_load(bf16x8 (&R)[NR], const Lds<G>& sm, const FusedP& p, int li, int g, int h, int b, int tdev, int lane) {
    const int r = lane >> 3, c = lane & 7;
    const unsigned kb = (unsigned)p.T * HD;
    const char* Kl = (const char*)(p.cache + (int64_t)(2 * li) * p.plane + (int64_t)h * p.T * 64);
    const char* Vl = (const char*)(p.cache + (int64_t)(2 * li + 1) * p.plane + (int64_t)h * p.T * 64);
#pragma unroll
    for (int i = 0; i < NIS; ++i) {
        const int j = 8 * i + r;
        const int rowi = (p.rows && j < tdev) ? sm.rt[g][j] : b;
        const unsigned off = ((unsigned)rowi * kb + (unsigned)min(j, tdev) * 64u + (unsigned)c * 8u) * 2u;     // < 2^32: checked on the host
        if (KEYS) R[i] = *(const bf16x8*)(Kl + off);
        if (VALUES) R[NIS + i] = *(const bf16x8*)(Vl + off);
    }
}
template <int G>
__device__ __forceinline__ void self_compute(bf16x8 (&R)[NR], Lds<G>& sm, const FusedP& p, int li, int g, int h, int b, int tdev, int lane, bool more) {
    const int r = lane >> 3, c = lane & 7;
    const bf16_t* fresh_k = &sm.wide[g][HD + h * 64];
    const bf16_t* fresh_v = &sm.wide[g][2 * HD + h * 64];
    {   // this step's key / value join the cache (used from LDS below, never read back from there in this launch)
        bf16_t* Kl = p.cache + (int64_t)(2 * li) * p.plane + (int64_t)h * p.T * 64;
        bf16_t* Vl = p.cache + (int64_t)(2 * li + 1) * p.plane + (int64_t)h * p.T * 64;
        const int64_t at = (int64_t)b * p.T * HD + (int64_t)tdev * 64 + lane;
        Kl[at] = fresh_k[lane]; Vl[at] = fresh_v[lane];
        if (p.rows && lane == 0 && h == 0) p.rows[(int64_t)b * p.T + tdev] = b;
    }
    const bf16x8 fk8 = *(const bf16x8*)(fresh_k + c * 8), fv8 = *(const bf16x8*)(fresh_v + c * 8);
    const u32x4_t qp = scaled_query(&sm.wide[g][h * 64 + c * 8]);
    float sc[NIS];
    float mx = -INFINITY;
#pragma unroll
    for (int i = 0; i < NIS; ++i) {
        const int j = 8 * i + r;
        bf16x8 kk = R[i];
        if (j == tdev) kk = fk8;
        const float a = sum8(dot8(kk, qp));
        sc[i] = (j <= tdev && sm.vf[g][j]) ? a : -INFINITY;
        mx = fmaxf(mx, sc[i]);
    }
    if (more) self_load<G, true, false>(R, sm, p, li, g + 1, h, b + 1, tdev, lane);       // the next sequence's keys: the key registers are free
    mx = wave_max_d(mx);
    const bool dead = mx == -INFINITY;               // no usable key (a finished, all-pad row): output zeros
    float sum = 0.f;
#pragma unroll
    for (int i = 0; i < NIS; ++i) { sc[i] = dead ? 0.f : __expf(sc[i] - mx); sum += sc[i]; }
    sum = wave_sum_d(sum) * 0.125f;                  // every key is counted by the 8 lanes of its row
    const float inv = dead ? 0.f : 1.f / sum;
    float o[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int i = 0; i < NIS; ++i) {
        const int j = 8 * i + r;
        bf16x8 vv = R[NIS + i];
        if (j == tdev) vv = fv8;
        if (j > tdev) vv = (bf16x8){0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
        for (int e = 0; e < 8; ++e) o[e] += sc[i] * bf2f((bf16_t)vv[e]);
    }
    if (more) self_load<G, false, true>(R, sm, p, li, g + 1, h, b + 1, tdev, lane);       // ... and its values
#pragma unroll
    for (int e = 0; e < 8; ++e) o[e] = sum_rows(o[e]);
    if (r == 0) {
        typedef __attribute__((ext_vector_type(4))) unsigned u32x4;
        *(u32x4*)(&sm.ctx[g][h * 64 + c * 8]) = (u32x4){pack_bf2(o[0] * inv, o[1] * inv), pack_bf2(o[2] * inv, o[3] * inv), pack_bf2(o[4] * inv, o[5] * inv), pack_bf2(o[6] * inv, o[7] * inv)};
    }
}
// ---- cross-attention over the image's patch keys of head h (shared by the G sequences): NC chunks of CI key iterations (8 keys each)
// through NB = max(NC / 2, 1) buffers of the role registers (2 CI fragments each: a chunk's keys, then its values).  NC = 1 is the
// instance for up to NPMAX keys: all NIC iterations in one pass, no carried state.  NC > 1 takes 161 .. NPWIDE keys, NIW iterations in
// all: chunk S lives in buffer S % NB; the chunks of the first NB are requested behind B2, chunk S + NB right behind the last use of
// chunk S, so with NB > 1 a chunk's rows travel while its neighbour is being used.  Per sequence the running maximum, the running sum
// and the lane's 8 unnormalised output sums are carried from chunk to chunk in LDS (each lane re-reads what it wrote itself: no
// barrier) with the usual rescale
//   m' = max(m, chunk maximum), l' = l e^(m - m') + sum e^(s - m'), o' = o e^(m - m') + sum e^(s - m') v
// and the last chunk reduces over the key rows, normalises and packs to bf16 once.  Chunk 0 holds key 0, so m is finite from the
// first chunk on and a chunk that lies wholly past npa (its loads clamped to the last row) adds exact zeros.
template <int G> struct CrossState { float v[G][NH][10][64]; };      // [8 output sums, m, l][lane]; NC > 1 only
constexpr int cross_iters(int NC) { return NC == 1 ? NIC : NIW; }      // key iterations of all NC chunks together
template <int NC, int S>
__device__ __forceinline__ void cross_chunk_load(bf16x8 (&R)[NR], const FusedP& p, int li, int img, int h, int lane) {
    constexpr int CI = cross_iters(NC) / NC, NB = NC > 1 ? NC / 2 : 1, BASE = (S % NB) * 2 * CI;
    static_assert(cross_iters(NC) % NC == 0 && 2 * CI * NB <= NR, "cross_chunk_load: buffers");
    const int r = lane >> 3, c = lane & 7;
    const char* Kc = (const char*)(p.ckv + (int64_t)(2 * li) * p.plane2 + ((int64_t)img * NH + h) * p.npa * 64);
    const char* Vc = (const char*)(p.ckv + (int64_t)(2 * li + 1) * p.plane2 + ((int64_t)img * NH + h) * p.npa * 64);
#pragma unroll
    for (int i = 0; i < CI; ++i) {
        const unsigned off = ((unsigned)min(8 * (S * CI + i) + r, p.npa - 1) * 64u + (unsigned)c * 8u) * 2u;  // past the last key: a real row, probability 0
        R[BASE + i] = *(const bf16x8*)(Kc + off);
        R[BASE + CI + i] = *(const bf16x8*)(Vc + off);
    }
}
template <int G, int NC, int S>      // st: null for NC = 1
__device__ __forceinline__ void cross_chunk_compute(bf16x8 (&R)[NR], Lds<G>& sm, CrossState<G>* st, const FusedP& p, int h, int lane) {
    constexpr int CI = cross_iters(NC) / NC, NB = NC > 1 ? NC / 2 : 1, BASE = (S % NB) * 2 * CI;
    const int r = lane >> 3, c = lane & 7;
#pragma unroll 1
    for (int g = 0; g < G; ++g) {
        // the rows are the same for every sequence: without this hipcc hoists their bf16 -> fp32 conversions out of the loop (and spills them)
#pragma unroll
        for (int i = 0; i < 2 * CI; ++i) asm volatile("" : "+v"(R[BASE + i]));
        const u32x4_t qp = scaled_query(&sm.wide[g][h * 64 + c * 8]);
        float* sv = NC > 1 ? &st->v[g][h][0][lane] : nullptr;
        float sc[CI];
        float mx = -INFINITY;
#pragma unroll
        for (int i = 0; i < CI; ++i) {
            const float a = sum8(dot8(R[BASE + i], qp));
            sc[i] = (8 * (S * CI + i) + r < p.npa) ? a : -INFINITY;
            mx = fmaxf(mx, sc[i]);
        }
        mx = wave_max_d(mx);
        float o[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        float l = 0.f;
        if constexpr (S > 0) {
            const float m0 = sv[8 * 64];
            mx = fmaxf(mx, m0);
            const float f = __expf(m0 - mx);
            l = sv[9 * 64] * f;
#pragma unroll
            for (int e = 0; e < 8; ++e) o[e] = sv[e * 64] * f;
        }
        float sum = 0.f;
#pragma unroll
        for (int i = 0; i < CI; ++i) { sc[i] = __expf(sc[i] - mx); sum += sc[i]; }
        // every key is counted by the 8 lanes of its row.  Two forms, so that neither family's code moves: `l +=` contracts to an FMA
        // (with l = 0 in chunk 0 too), which the one-pass instances never had
        if constexpr (NC == 1) l = wave_sum_d(sum) * 0.125f;
        else l += wave_sum_d(sum) * 0.125f;
#pragma unroll
        for (int i = 0; i < CI; ++i)
#pragma unroll
            for (int e = 0; e < 8; ++e) o[e] += sc[i] * bf2f((bf16_t)R[BASE + CI + i][e]);
        if constexpr (S + 1 < NC) {
#pragma unroll
            for (int e = 0; e < 8; ++e) sv[e * 64] = o[e];
            sv[8 * 64] = mx; sv[9 * 64] = l;
        } else {
            const float inv = 1.f / l;
#pragma unroll
            for (int e = 0; e < 8; ++e) o[e] = sum_rows(o[e]);
            if (r == 0) {
                typedef __attribute__((ext_vector_type(4))) unsigned u32x4;
                *(u32x4*)(&sm.ctx[g][h * 64 + c * 8]) = (u32x4){pack_bf2(o[0] * inv, o[1] * inv), pack_bf2(o[2] * inv, o[3] * inv), pack_bf2(o[4] * inv, o[5] * inv), pack_bf2(o[6] * inv, o[7] * inv)};
            }
        }
    }
}
// chunks S .. NC - 1 in turn: use chunk S, then request chunk S + NB into the buffer it leaves
template <int G, int NC, int S>
__device__ __forceinline__ void cross_chunks(bf16x8 (&R)[NR], Lds<G>& sm, CrossState<G>* st, const FusedP& p, int li, int img, int h, int lane0) {
    constexpr int NB = NC > 1 ? NC / 2 : 1;
    cross_chunk_compute<G, NC, S>(R, sm, st, p, h, opaque(lane0));
    if constexpr (NC > 1) { DF_STAMP_A(8 + S); }
    if constexpr (S + NB < NC) cross_chunk_load<NC, S + NB>(R, p, li, img, h, opaque(lane0));
    if constexpr (S + 1 < NC) cross_chunks<G, NC, S + 1>(R, sm, st, p, li, img, h, lane0);
}
// biases + LayerNorm weights of one layer -> LDS (256 threads; the loads go out together, one wait, then the writes)
__device__ __forceinline__ void params_load(float* par, const FusedLayer& L, int t256_) {
    const int t256 = opaque(t256_);
    const float* src[12] = {L.bqkv, L.bo, L.bcq, L.bco, L.bfc1, L.bfc2, L.ln1w, L.ln1b, L.ln2w, L.ln2b, L.ln3w, L.ln3b};
    const int dst[12] = {PB_QKV, PB_O, PB_CQ, PB_CO, PB_FC1, PB_FC2, PL1W, PL1B, PL2W, PL2B, PL3W, PL3B};
    const int n4[12] = {192, 64, 64, 64, 192, 64, 64, 64, 64, 64, 64, 64};
    float4 v[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) v[k] = ((const float4*)src[k])[min(t256, n4[k] - 1)];
#pragma unroll
    for (int k = 0; k < 12; ++k) if (t256 < n4[k]) *(float4*)(par + dst[k] + t256 * 4) = v[k];
}

// a layer's row scales (e4m3 instances) -> LDS, likewise; n4 = SCL / 4, or 64 for the head's dense layer
__device__ __forceinline__ void scales_load(float* scl, const float* src, int n4, int t256_) {
    const int t256 = opaque(t256_);
    float4 v[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) v[k] = ((const float4*)src)[min(t256 + 256 * k, n4 - 1)];
#pragma unroll
    for (int k = 0; k < 3; ++k) if (t256 + 256 * k < n4) *(float4*)(scl + (t256 + 256 * k) * 4) = v[k];
}

// ---- the two roles: each runs its own layer loop; the barrier sequences match (1 + 11 per layer) -------------------------------
template <int G, bool F8>       // F8: the weights come from the e4m3 stream (rows_gemm8), scl = the row scales the attention waves put in LDS
__device__ __forceinline__ void linear_role(Lds<G>& sm, float (*scl)[SCL], const typename FusedArgs<F8>::type& p, int w, int lane0, int b0) {
    bf16x8 R[NR];                                     // only R[0 .. WIN) is used here: the weight window
    const char* sb = nullptr;                         // the wave's e4m3 stream at the current layer
    if constexpr (F8) sb = p.w8 + (int64_t)w * p.wave8;
    {
        // embeddings: x0 = LN(word[token] + type[0] + position[posid]) (modeling_roberta.py:75-122); requested BEFORE the window
        const int lane = opaque(lane0);
        float4 wv = make_float4(0, 0, 0, 0), ty = wv, pv = wv, ga = wv, be = wv;
        if (w < G) {
            const int64_t id = p.tokens[b0 + w];
            const int pid = p.posids[b0 + w];
            wv = *(const float4*)(p.word + id * HD + lane * 4); ty = *(const float4*)(p.type0 + lane * 4);
            pv = *(const float4*)(p.postab + (int64_t)pid * HD + lane * 4);
            ga = *(const float4*)(p.elnw + lane * 4); be = *(const float4*)(p.elnb + lane * 4);
        }
        if constexpr (F8) fill_window8(R, sb, lane);
        else fill_window<6, 8, NLW, WIN>(R, wave_frags<6, 8>(p.L[0].wqkv, w), lane);
        if (w < G) {
            const float4 v = make_float4(wv.x + ty.x + pv.x, wv.y + ty.y + pv.y, wv.z + ty.z + pv.z, wv.w + ty.w + pv.w);
            const float mean = wave_sum(v.x + v.y + v.z + v.w) * (1.f / HD);
            const float a = v.x - mean, b = v.y - mean, c = v.z - mean, d = v.w - mean;
            const float rstd = rsqrtf(wave_sum(a * a + b * b + c * c + d * d) * (1.f / HD) + p.eps);
            const float y0 = a * rstd * ga.x + be.x, y1 = b * rstd * ga.y + be.y, y2 = c * rstd * ga.z + be.z, y3 = d * rstd * ga.w + be.w;
            *(float4*)(&sm.xs[w][lane * 4]) = make_float4(y0, y1, y2, y3);
            *(uint2*)(&sm.ab[w][lane * 4]) = make_uint2(pack_bf2(y0, y1), pack_bf2(y2, y3));
        }
    }
    wg_barrier();
    DF_STAMP(1);
    for (int li = 0; li < p.nlayers; ++li) {
        const FusedLayer& L = p.L[li];
        const float* par = sm.par[li & 1];
        const float* sc = F8 ? scl[li & 1] : nullptr;
        DF_STAMP_L(0);
        {   // q | k | v = x Wqkv^T + b, in two column halves (24 accumulator registers instead of 48: the window gets them)
            const int lane = opaque(lane0), l15 = lane & 15, g4 = lane >> 4;
#pragma unroll
            for (int half = 0; half < 2; ++half) {
                f32x4 acc[6];
                if constexpr (F8) { if (half == 0) rows_gemm8<6, 8, S8_QKV, G>(R, sb, &sm.ab[0][0], LDH, lane, acc); else rows_gemm8<6, 8, S8_QKV + 24, G>(R, sb, &sm.ab[0][0], LDH, lane, acc); }
                else if (half == 0) rows_gemm<6, 8, 6, 8, 0, G>(R, wave_frags<6, 8>(L.wqkv, w), wave_frags<6, 8>(L.wqkv, w + 24), &sm.ab[0][0], LDH, lane, acc);
                else rows_gemm<6, 8, 4, 8, 48 % WIN, G>(R, wave_frags<6, 8>(L.wqkv, w + 24), wave_frags<4, 8>(L.wo, w), &sm.ab[0][0], LDH, lane, acc);
                if (l15 < G) {
#pragma unroll
                    for (int cb = 0; cb < 6; ++cb) {
                        const int n = (w + 4 * (cb + 6 * half)) * 16 + 4 * g4;
                        const float4 bb = *(const float4*)(par + PB_QKV + n), s4 = scale4<F8>(sc, PB_QKV + n);
                        *(uint2*)(&sm.wide[l15][n]) = make_uint2(pack_bf2(sb_add<F8>(acc[cb][0], s4.x, bb.x), sb_add<F8>(acc[cb][1], s4.y, bb.y)),
                                                                 pack_bf2(sb_add<F8>(acc[cb][2], s4.z, bb.z), sb_add<F8>(acc[cb][3], s4.w, bb.w)));
                    }
                }
            }
        }
        wg_barrier();            // B1
        DF_STAMP_L(1);
        wg_barrier();            // B2: self-attention done
        DF_STAMP_L(2);
        {   // s1 = ctx Wo^T + b + x
            const int lane = opaque(lane0), l15 = lane & 15, g4 = lane >> 4;
            f32x4 acc[4];
            if constexpr (F8) rows_gemm8<4, 8, S8_O, G>(R, sb, &sm.ctx[0][0], LDH, lane, acc);
            else rows_gemm<4, 8, 4, 8, (12 * 8) % WIN, G>(R, wave_frags<4, 8>(L.wo, w), wave_frags<4, 8>(L.wcq, w), &sm.ctx[0][0], LDH, lane, acc);
            if (l15 < G) {
#pragma unroll
                for (int cb = 0; cb < 4; ++cb) {
                    const int n = (w + 4 * cb) * 16 + 4 * g4;
                    const float4 bb = *(const float4*)(par + PB_O + n), x4 = *(const float4*)(&sm.xs[l15][n]), s4 = scale4<F8>(sc, PB_O + n);
                    *(float4*)(&sm.ss[l15][n]) = make_float4(sb_add<F8>(acc[cb][0], s4.x, bb.x) + x4.x, sb_add<F8>(acc[cb][1], s4.y, bb.y) + x4.y,
                                                             sb_add<F8>(acc[cb][2], s4.z, bb.z) + x4.z, sb_add<F8>(acc[cb][3], s4.w, bb.w) + x4.w);
                }
            }
        }
        wg_barrier();            // B3
        DF_STAMP_L(3);
        if (w < G) ln_row(sm.ss[w], par + PL1W, par + PL1B, p.eps, sm.xs[w], sm.ab[w], opaque(lane0));
        wg_barrier();            // B4
        DF_STAMP_L(4);
        {   // cross query
            const int lane = opaque(lane0), l15 = lane & 15, g4 = lane >> 4;
            f32x4 acc[4];
            if constexpr (F8) rows_gemm8<4, 8, S8_CQ, G>(R, sb, &sm.ab[0][0], LDH, lane, acc);
            else rows_gemm<4, 8, 4, 8, (12 * 8 + 32) % WIN, G>(R, wave_frags<4, 8>(L.wcq, w), wave_frags<4, 8>(L.wco, w), &sm.ab[0][0], LDH, lane, acc);
            if (l15 < G) {
#pragma unroll
                for (int cb = 0; cb < 4; ++cb) {
                    const int n = (w + 4 * cb) * 16 + 4 * g4;
                    const float4 bb = *(const float4*)(par + PB_CQ + n), s4 = scale4<F8>(sc, PB_CQ + n);
                    *(uint2*)(&sm.wide[l15][n]) = make_uint2(pack_bf2(sb_add<F8>(acc[cb][0], s4.x, bb.x), sb_add<F8>(acc[cb][1], s4.y, bb.y)),
                                                             pack_bf2(sb_add<F8>(acc[cb][2], s4.z, bb.z), sb_add<F8>(acc[cb][3], s4.w, bb.w)));
                }
            }
        }
        wg_barrier();            // B5
        DF_STAMP_L(5);
        wg_barrier();            // B6: cross-attention done
        DF_STAMP_L(6);
        {   // s2 = cctx Wco^T + b + x
            const int lane = opaque(lane0), l15 = lane & 15, g4 = lane >> 4;
            f32x4 acc[4];
            if constexpr (F8) rows_gemm8<4, 8, S8_CO, G>(R, sb, &sm.ctx[0][0], LDH, lane, acc);
            else rows_gemm<4, 8, 6, 8, (12 * 8 + 64) % WIN, G>(R, wave_frags<4, 8>(L.wco, w), wave_frags<6, 8>(L.wfc1, w), &sm.ctx[0][0], LDH, lane, acc);
            if (l15 < G) {
#pragma unroll
                for (int cb = 0; cb < 4; ++cb) {
                    const int n = (w + 4 * cb) * 16 + 4 * g4;
                    const float4 bb = *(const float4*)(par + PB_CO + n), x4 = *(const float4*)(&sm.xs[l15][n]), s4 = scale4<F8>(sc, PB_CO + n);
                    *(float4*)(&sm.ss[l15][n]) = make_float4(sb_add<F8>(acc[cb][0], s4.x, bb.x) + x4.x, sb_add<F8>(acc[cb][1], s4.y, bb.y) + x4.y,
                                                             sb_add<F8>(acc[cb][2], s4.z, bb.z) + x4.z, sb_add<F8>(acc[cb][3], s4.w, bb.w) + x4.w);
                }
            }
        }
        wg_barrier();            // B7
        DF_STAMP_L(7);
        if (w < G) ln_row(sm.ss[w], par + PL2W, par + PL2B, p.eps, sm.xs[w], sm.ab[w], opaque(lane0));
        wg_barrier();            // B8
        DF_STAMP_L(8);
        {   // FFN: act = gelu(x Wfc1^T + b), in two column halves
            const int lane = opaque(lane0), l15 = lane & 15, g4 = lane >> 4;
#pragma unroll
            for (int half = 0; half < 2; ++half) {
                f32x4 acc[6];
                if constexpr (F8) { if (half == 0) rows_gemm8<6, 8, S8_FC1, G>(R, sb, &sm.ab[0][0], LDH, lane, acc); else rows_gemm8<6, 8, S8_FC1 + 24, G>(R, sb, &sm.ab[0][0], LDH, lane, acc); }
                else if (half == 0) rows_gemm<6, 8, 6, 8, (96 + 96) % WIN, G>(R, wave_frags<6, 8>(L.wfc1, w), wave_frags<6, 8>(L.wfc1, w + 24), &sm.ab[0][0], LDH, lane, acc);
                else rows_gemm<6, 8, 4, 24, (96 + 96 + 48) % WIN, G>(R, wave_frags<6, 8>(L.wfc1, w + 24), wave_frags<4, 24>(L.wfc2, w), &sm.ab[0][0], LDH, lane, acc);
                if (l15 < G) {
#pragma unroll
                    for (int cb = 0; cb < 6; ++cb) {
                        const int n = (w + 4 * (cb + 6 * half)) * 16 + 4 * g4;
                        const float4 bb = *(const float4*)(par + PB_FC1 + n), s4 = scale4<F8>(sc, PB_FC1 + n);
                        float y[4], d;
                        gelu_erf_both(sb_add<F8>(acc[cb][0], s4.x, bb.x), &y[0], &d); gelu_erf_both(sb_add<F8>(acc[cb][1], s4.y, bb.y), &y[1], &d);
                        gelu_erf_both(sb_add<F8>(acc[cb][2], s4.z, bb.z), &y[2], &d); gelu_erf_both(sb_add<F8>(acc[cb][3], s4.w, bb.w), &y[3], &d);
                        *(uint2*)(&sm.wide[l15][n]) = make_uint2(pack_bf2(y[0], y[1]), pack_bf2(y[2], y[3]));
                    }
                }
            }
        }
        wg_barrier();            // B9
        DF_STAMP_L(9);
        {   // s3 = act Wfc2^T + b + x
            const int lane = opaque(lane0), l15 = lane & 15, g4 = lane >> 4;
            f32x4 acc[4];
            if constexpr (F8) { rows_gemm8<4, 24, S8_FC2, G>(R, sb, &sm.wide[0][0], LDW, lane, acc); sb += S8_LAYER * 1024; }
            else if (li + 1 < p.nlayers) rows_gemm<4, 24, 6, 8, (12 * 8 + 96 + 96) % WIN, G>(R, wave_frags<4, 24>(L.wfc2, w), wave_frags<6, 8>(p.L[li + 1].wqkv, w), &sm.wide[0][0], LDW, lane, acc);
            else rows_gemm<4, 24, 4, 8, (12 * 8 + 96 + 96) % WIN, G>(R, wave_frags<4, 24>(L.wfc2, w), wave_frags<4, 8>(p.whd, w), &sm.wide[0][0], LDW, lane, acc);
            if (l15 < G) {
#pragma unroll
                for (int cb = 0; cb < 4; ++cb) {
                    const int n = (w + 4 * cb) * 16 + 4 * g4;
                    const float4 bb = *(const float4*)(par + PB_FC2 + n), x4 = *(const float4*)(&sm.xs[l15][n]), s4 = scale4<F8>(sc, PB_FC2 + n);
                    *(float4*)(&sm.ss[l15][n]) = make_float4(sb_add<F8>(acc[cb][0], s4.x, bb.x) + x4.x, sb_add<F8>(acc[cb][1], s4.y, bb.y) + x4.y,
                                                             sb_add<F8>(acc[cb][2], s4.z, bb.z) + x4.z, sb_add<F8>(acc[cb][3], s4.w, bb.w) + x4.w);
                }
            }
        }
        wg_barrier();            // B10
        DF_STAMP_L(10);
        if (w < G) ln_row(sm.ss[w], par + PL3W, par + PL3B, p.eps, sm.xs[w], sm.ab[w], opaque(lane0));
        wg_barrier();            // B11
        DF_STAMP_L(11);
    }
    DF_STAMP(40);
    {   // LM head, first half: gelu(x Wd^T + b) in fp32 (its LayerNorm and the vocabulary GEMM are the next launch)
        const int lane = opaque(lane0), l15 = lane & 15, g4 = lane >> 4;
        const float* par = sm.par[p.nlayers & 1];
        const float* sc = F8 ? scl[p.nlayers & 1] : nullptr;
        f32x4 acc[4];
        if constexpr (F8) rows_gemm8<4, 8, 0, G>(R, sb, &sm.ab[0][0], LDH, lane, acc);
        else rows_gemm<4, 8, 4, 8, 0, G>(R, wave_frags<4, 8>(p.whd, w), nullptr, &sm.ab[0][0], LDH, lane, acc);
        if (l15 < G) {
#pragma unroll
            for (int cb = 0; cb < 4; ++cb) {
                const int n = (w + 4 * cb) * 16 + 4 * g4;
                const float4 bb = *(const float4*)(par + n), s4 = scale4<F8>(sc, n);
                float y[4], d;
                gelu_erf_both(sb_add<F8>(acc[cb][0], s4.x, bb.x), &y[0], &d); gelu_erf_both(sb_add<F8>(acc[cb][1], s4.y, bb.y), &y[1], &d);
                gelu_erf_both(sb_add<F8>(acc[cb][2], s4.z, bb.z), &y[2], &d); gelu_erf_both(sb_add<F8>(acc[cb][3], s4.w, bb.w), &y[3], &d);
                *(float4*)(p.hd_out + (int64_t)(b0 + l15) * HD + n) = make_float4(y[0], y[1], y[2], y[3]);
            }
        }
    }
    DF_STAMP(41);
}

template <int G, int NC, bool F8>
__device__ __forceinline__ void attention_role(Lds<G>& sm, float (*scl)[SCL], const typename FusedArgs<F8>::type& p, int h, int lane0, int t256, int img, int b0, int tdev) {
    bf16x8 R[NR];                                     // key + value rows
    {   // layer 0's biases / LayerNorm weights, the sequences' row table and usable-key flags -> LDS
        const int lane = opaque(lane0);
        params_load(sm.par[0], p.L[0], t256);
        if constexpr (F8) scales_load(scl[0], p.sc8, SCL / 4, t256);
        for (int g = h; g < G; g += 4) {
            const int b = b0 + g;
#pragma unroll
            for (int q = 0; q < TMAX / 64; ++q) {
                const int j = lane + 64 * q;
                sm.rt[g][j] = p.rows ? p.rows[(int64_t)b * p.T + min(j, p.T - 1)] : b;
                sm.vf[g][j] = p.valid ? p.valid[(int64_t)b * p.ldvalid + min(j, (int)p.ldvalid - 1)] : (unsigned char)1;
            }
        }
    }
    wg_barrier();
    self_load<G, true, true>(R, sm, p, 0, 0, h, b0, tdev, opaque(lane0));       // in flight while the first QKV projection runs
    for (int li = 0; li < p.nlayers; ++li) {
        wg_barrier();            // B1: q | k | v of this step are in LDS
        DF_STAMP_A(0);
        {   // cached self-attention of head h for every sequence; then the image's patch keys / values are requested
            const int lane = opaque(lane0);
#pragma unroll 1
            for (int g = 0; g < G; ++g) {             // sequence g + 1's rows are requested while sequence g's are being used
                self_compute<G>(R, sm, p, li, g, h, b0 + g, tdev, lane, g + 1 < G);
                DF_STAMP_A(1);
            }
            DF_STAMP_A(2);
        }
        wg_barrier();            // B2: the attention output is in LDS; the image's patch keys / values are requested behind it
        cross_chunk_load<NC, 0>(R, p, li, img, h, opaque(lane0));                      // the chunks of the first NB buffers
        if constexpr (NC >= 4) cross_chunk_load<NC, 1>(R, p, li, img, h, opaque(lane0));
        if constexpr (NC >= 8) { cross_chunk_load<NC, 2>(R, p, li, img, h, opaque(lane0)); cross_chunk_load<NC, 3>(R, p, li, img, h, opaque(lane0)); }
        DF_STAMP_A(3);
        wg_barrier();            // B3
        wg_barrier();            // B4
        wg_barrier();            // B5: the cross query is in LDS
        DF_STAMP_A(4);
        {   // cross-attention of head h for every sequence; then the next layer's parameters and its first cached rows
            CrossState<G>* st = nullptr;
            if constexpr (NC > 1) { __shared__ CrossState<G> st_s; st = &st_s; }      // the chunked instances only
            cross_chunks<G, NC, 0>(R, sm, st, p, li, img, h, lane0);
            DF_STAMP_A(5);
        }
        wg_barrier();            // B6: the cross-attention output is in LDS; behind it, the next layer's parameters and first cached rows
        if (li + 1 < p.nlayers) {
            params_load(sm.par[(li + 1) & 1], p.L[li + 1], t256);
            if constexpr (F8) scales_load(scl[(li + 1) & 1], p.sc8 + (int64_t)(li + 1) * SCL, SCL / 4, t256);
            DF_STAMP_A(6);
            self_load<G, true, true>(R, sm, p, li + 1, 0, h, b0, tdev, opaque(lane0));
            DF_STAMP_A(7);
        } else if (opaque(t256) < 64) {
            *(float4*)(sm.par[(li + 1) & 1] + opaque(t256) * 4) = ((const float4*)p.bhd)[opaque(t256)];      // the LM head dense layer's bias
            if constexpr (F8) *(float4*)(scl[(li + 1) & 1] + opaque(t256) * 4) = ((const float4*)(p.sc8 + (int64_t)(li + 1) * SCL))[opaque(t256)];      // ... and its row scales
        }
        wg_barrier();            // B7
        wg_barrier();            // B8
        wg_barrier();            // B9
        wg_barrier();            // B10
        wg_barrier();            // B11
    }
}

// NC = 1: up to NPMAX patch keys in one pass; NC > 1: up to NPWIDE in NC chunks; F8: e4m3 weights; SL: the workgroup is a decoder
// SLOT -- its image and its step index are two scalar loads at the top (an idle slot leaves before the first barrier: the test is
// workgroup-uniform), tokens / position ids / head output / self-attention cache stay indexed by the slot's rows b0 .. b0 + G - 1.  Every
// step costs the same at every t and cache rows past t are never used (self_load, self_compute), so a slot restarts at t = 0 without any
// clean-up.  A slot of G = 2 / 4 rows holds an image's beam group and reads the beam row table: self_load takes an entry only for
// j < tdev, so the entries a reseated slot inherits from the image before are never used either, and self_compute writes
// rows[b][tdev] = b before the update kernel re-parents columns 0 .. tdev in place -- the table needs no clean-up at a reseat.
template <int G, int NC, bool F8, bool SL = false>
__global__ __launch_bounds__(512) void decode_fused_kernel(const typename FusedArgs<F8, SL>::type p) {
    __shared__ Lds<G> sm;
    float (*scl)[SCL] = nullptr;                         // the layer's / the next layer's row scales: the e4m3 instances only
    if constexpr (F8) { __shared__ float scl_s[2][SCL]; scl = scl_s; }
    const int tid = threadIdx.x, lane0 = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6);
    static_assert(!SL || G == 1 || G == 2 || G == 4, "a slot holds one sequence or an image's 2 / 4 beams");
    const int b0 = blockIdx.x * G;
    int img = blockIdx.x, tdev;
    if constexpr (SL) {
        img = p.slot_image[blockIdx.x]; tdev = min(p.slot_t[blockIdx.x], p.T - 1);
        if (img < 0) return;
    } else tdev = p.tptr ? min(*p.tptr, p.T - 1) : p.t;
    static_assert((12 * 8 + 3 * 32 + 2 * 96) % WIN == 0, "a layer's fragments must fill the window a whole number of times");
    DF_STAMP(0);
    if (w < 4) linear_role<G, F8>(sm, scl, p, w, lane0, b0);
    else attention_role<G, NC, F8>(sm, scl, p, w - 4, lane0, tid - 256, img, b0, tdev);
}

}  // namespace

#ifdef KZV_STAMPS
extern "C" int kzv_debug_decode_stamps(long long* host, int n) {
    return hipMemcpyFromSymbol(host, HIP_SYMBOL(g_df_stamps), sizeof(long long) * (n < 64 ? n : 64)) == hipSuccess ? 0 : 1;
}
#endif

int kzv_decode_fused_supported(int Hd, int heads, int Fd, int layers, int group, int T, int npa) {
    return Hd == HD && heads == NH && Fd == FD && layers >= 1 && layers <= KZV_DECODE_FUSED_MAX_LAYERS && (group == 1 || group == 2 || group == 4) &&
           T >= 1 && T <= TMAX && npa >= 1 && npa <= NPWIDE;
}

int kzv_decode_fused_launch(const KzvDecodeFused& a, hipStream_t s) {
    if (!kzv_decode_fused_supported(HD, NH, FD, a.nlayers, a.group, a.T, a.npa)) return kzv_fail(KZV_E_ARG, "decode_fused: geometry not instantiated");
    if (a.B % a.group) return kzv_fail(KZV_E_ARG, "decode_fused: rows must be a multiple of the group");
    if ((a.rows || a.slot_image) && (int64_t)a.B * a.T * HD >= (1ll << 31)) return kzv_fail(KZV_E_ARG, "decode_fused: cache too large");
    if ((a.slot_image == nullptr) != (a.slot_t == nullptr)) return kzv_fail(KZV_E_ARG, "decode_fused: a slot's image and step tables go together");
    if (a.slot_image && (a.valid || a.tptr)) return kzv_fail(KZV_E_ARG, "decode_fused: slots take no key flags and no launch-wide step");
    if (a.slot_image && (a.group == 1) != (a.rows == nullptr)) return kzv_fail(KZV_E_ARG, "decode_fused: a slot is one greedy sequence without a row table, or a beam group of 2 / 4 with one");
    FusedP p;
    for (int i = 0; i < a.nlayers; ++i) {
        const KzvDecodeFusedLayer& l = a.layers[i];
        p.L[i] = FusedLayer{l.wqkv, l.wo, l.wcq, l.wco, l.wfc1, l.wfc2, l.bqkv, l.bo, l.bcq, l.bco, l.bfc1, l.bfc2, l.ln1w, l.ln1b, l.ln2w, l.ln2b, l.ln3w, l.ln3b};
    }
    for (int i = a.nlayers; i < KZV_DECODE_FUSED_MAX_LAYERS; ++i) p.L[i] = p.L[0];
    p.nlayers = a.nlayers; p.tokens = a.tokens; p.posids = a.posids; p.word = a.word; p.type0 = a.type0; p.postab = a.postab; p.elnw = a.elnw; p.elnb = a.elnb;
    p.whd = a.whd; p.bhd = a.bhd; p.hd_out = a.hd_out; p.cache = a.cache; p.plane = a.plane; p.ckv = a.ckv; p.plane2 = a.plane2;
    p.valid = a.valid; p.ldvalid = a.ldvalid; p.tptr = a.tptr; p.t = a.t; p.T = a.T; p.npa = a.npa; p.B = a.B; p.rows = a.rows; p.eps = a.eps;
    if ((a.w8 == nullptr) != (a.scales8 == nullptr)) return kzv_fail(KZV_E_ARG, "decode_fused: the e4m3 stream and its row scales go together");
    const int images = a.B / a.group;
    // up to NPMAX keys: the one-pass instances (a chunk that held no key at all would be all -inf); beyond: the chunked ones
    const bool wide = a.npa > NPMAX;
#define KZV_DF_PICK(F8_) (!wide ? (a.group == 1 ? decode_fused_kernel<1, 1, F8_> : a.group == 2 ? decode_fused_kernel<2, 1, F8_> : decode_fused_kernel<4, 1, F8_>) \
                                : (a.group == 1 ? decode_fused_kernel<1, KZV_DF_CHUNKS, F8_> : a.group == 2 ? decode_fused_kernel<2, KZV_DF_CHUNKS, F8_> : decode_fused_kernel<4, KZV_DF_CHUNKS, F8_>))
#define KZV_DF_PICK_SL(F8_) (!wide ? (a.group == 1 ? decode_fused_kernel<1, 1, F8_, true> : a.group == 2 ? decode_fused_kernel<2, 1, F8_, true> : decode_fused_kernel<4, 1, F8_, true>) \
                                   : (a.group == 1 ? decode_fused_kernel<1, KZV_DF_CHUNKS, F8_, true> : a.group == 2 ? decode_fused_kernel<2, KZV_DF_CHUNKS, F8_, true> : decode_fused_kernel<4, KZV_DF_CHUNKS, F8_, true>))
    if (a.slot_image) {
        if (a.w8) {
            FusedPS8 ps;
            static_cast<FusedP&>(ps) = p;
            ps.w8 = (const char*)a.w8; ps.wave8 = kzv_decode_fused_pack8_bytes(a.nlayers) / 4; ps.sc8 = a.scales8;
            ps.slot_image = a.slot_image; ps.slot_t = a.slot_t;
            void (*kern)(const FusedPS8) = KZV_DF_PICK_SL(true);
            hipLaunchKernelGGL(kern, dim3(images), dim3(512), 0, s, ps);
        } else {
            FusedPS ps;
            static_cast<FusedP&>(ps) = p;
            ps.slot_image = a.slot_image; ps.slot_t = a.slot_t;
            void (*kern)(const FusedPS) = KZV_DF_PICK_SL(false);
            hipLaunchKernelGGL(kern, dim3(images), dim3(512), 0, s, ps);
        }
    } else if (a.w8) {
        FusedP8 p8;
        static_cast<FusedP&>(p8) = p;
        p8.w8 = (const char*)a.w8; p8.wave8 = kzv_decode_fused_pack8_bytes(a.nlayers) / 4; p8.sc8 = a.scales8;
        void (*kern)(const FusedP8) = KZV_DF_PICK(true);
        hipLaunchKernelGGL(kern, dim3(images), dim3(512), 0, s, p8);
    } else {
        void (*kern)(const FusedP) = KZV_DF_PICK(false);
        hipLaunchKernelGGL(kern, dim3(images), dim3(512), 0, s, p);
    }
#undef KZV_DF_PICK_SL
#undef KZV_DF_PICK
    return kzv_check_launch("decode_fused");
}

// ---- the e4m3 copies ------------------------------------------------------------------------------------------------------------
int64_t kzv_decode_fused_pack8_bytes(int layers) { return (int64_t)4 * (S8_LAYER * layers + S8_HEAD + WIN8) * 1024; }
int64_t kzv_decode_fused_scales8(int layers) { return (int64_t)SCL * layers + HD; }

static int quant8_launch(Quant8Table& tab, hipStream_t s) {
    const int pad_blocks = tab.pad_pos >= 0 ? (4 * WIN8 * 64 + 255) / 256 : 0;
    hipLaunchKernelGGL(quant_pack8_kernel, dim3(tab.rows / 4 + pad_blocks), dim3(256), 0, s, tab);
    return kzv_check_launch("quant_pack8");
}

int kzv_decode_fused_pack8(const KzvDecodeFused8Src* layers, int nlayers, const bf16_t* whd, unsigned char* stream, float* scales, hipStream_t s) {
    if (!layers || !whd || !stream || !scales || nlayers < 1 || nlayers > KZV_DECODE_FUSED_MAX_LAYERS) return kzv_fail(KZV_E_ARG, "decode_fused_pack8: bad argument");
    Quant8Table tab;
    tab.n = 0; tab.rows = 0;
    const auto add = [&](const bf16_t* src, int N, int K, int scale_at, int cb, int pos) {
        tab.d[tab.n++] = Quant8Desc{src, N, K, tab.rows, scale_at, cb, pos};
        tab.rows += N;
    };
    for (int i = 0; i < nlayers; ++i) {
        const KzvDecodeFused8Src& l = layers[i];
        const int at = i * SCL, pos = i * S8_LAYER;
        add(l.wqkv, 3 * HD, HD, at + PB_QKV, 6, pos + S8_QKV); add(l.wo, HD, HD, at + PB_O, 4, pos + S8_O);
        add(l.wcq, HD, HD, at + PB_CQ, 4, pos + S8_CQ); add(l.wco, HD, HD, at + PB_CO, 4, pos + S8_CO);
        add(l.wfc1, FD, HD, at + PB_FC1, 6, pos + S8_FC1); add(l.wfc2, HD, FD, at + PB_FC2, 4, pos + S8_FC2);
    }
    add(whd, HD, HD, nlayers * SCL, 4, nlayers * S8_LAYER);
    tab.pad_pos = nlayers * S8_LAYER + S8_HEAD; tab.dst = stream; tab.scales = scales; tab.wave_bytes = kzv_decode_fused_pack8_bytes(nlayers) / 4;
    return quant8_launch(tab, s);
}

extern "C" int kzv_quant_pack_e4m3(const void* w_bf16, int N, int K, void* q_out, float* scale_out, void* stream) {
    if (!w_bf16 || !q_out || !scale_out) return kzv_fail(KZV_E_ARG, "quant_pack_e4m3: null operand");
    if (N < 16 || K < 64 || N % 16 || K % 64) return kzv_fail(KZV_E_ARG, "quant_pack_e4m3: N %% 16, K %% 64");
    if ((int64_t)N * K >= (1ll << 31)) return kzv_fail(KZV_E_ARG, "quant_pack_e4m3: matrix too large");
    Quant8Table tab;
    tab.d[0] = Quant8Desc{(const bf16_t*)w_bf16, N, K, 0, 0, 0, 0};
    tab.n = 1; tab.rows = N; tab.pad_pos = -1; tab.dst = (unsigned char*)q_out; tab.scales = scale_out; tab.wave_bytes = 0;
    return quant8_launch(tab, (hipStream_t)stream);
}
