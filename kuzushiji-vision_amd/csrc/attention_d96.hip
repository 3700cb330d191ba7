// Multi-head attention forward / backward for head_dim 96, no mask (ViT self-attention), Sq, Sk <= 288, bf16 MFMA.
//
// The reference CLI's default encoder (hidden 768, 8 heads on 1024 x 64 columns: 257 tokens, scripts/train_trocr.py:39-44) has
// 96-wide heads.  Same contract as the VALU kernel of attention_generic.hip (the two are interchangeable inside a run): the same
// kzv_attn_args, head h at column h * 96, scale 96^-0.5 in fp32, natural-log LSE [B, heads, Sq], the dropout masks of the packed
// 4 x 4-block generator of kzv_common.h; O / dQ / dK / dV are written, not accumulated.  No device scratch, no host synchronisation.
//
// The decomposition is attention.hip's (one workgroup per (batch, head), K and V of the head resident in LDS, S^T with the key on
// the accumulator rows in forward, key tiles owned by waves in backward), widened to D = 96:
//   * Q.K^T is three K-steps of v_mfma_f32_16x16x32_bf16, P.V six 16-column output tiles.
//   * LDS rows are 192 bytes (12 16-byte chunks).  Chunk c of row r sits at slot c ^ swz(r), swz(r) = the two bits (r >> 2) & 3
//     swapped.  Row reads (16 rows r0 .. r0 + 15, one chunk) land on 16 distinct bank slots; transposed reads (4-row blocks at
//     rows 4g + q of a 16-aligned base, 2 chunks) put the two 16-lane groups of a half on disjoint slots: both conflict-free.
//   * 8 waves per workgroup: the K and V images of 288 rows (108 KiB forward, 152 KiB of LDS in all backward) leave one
//     workgroup per CU, so 8 waves keep two per SIMD.
//   * Backward: Q and dO come in 32-query slabs through a 2-deep LDS ring, loaded into registers one slab ahead (plain loads,
//     retired by an explicit vmcnt(0) before they are written to LDS); dS^T crosses LDS for dQ as in attention.hip.
// The image layout (swz / img_off / tr_off<96>), the dropout bookkeeping and the per-tile / per-element steps are attention_common.h's.
// Every global load is unconditional (rows past the end are clamped or read the zero page); K / V use the builtin LDS-DMA, whose
// M0 the compiler owns.
#include "attention_common.h"

namespace {

constexpr int NW = 8, NT = NW * 64;     // waves, threads per workgroup
constexpr int NKT = 18, SP = NKT * 16;  // key tiles of 16 / image rows (288 tokens)
static_assert(SP == KZV_ATTN_MAX_S, "the images hold the longest sequence the dispatch sends here");
constexpr int NKP = NKT / 2;            // 32-key steps
constexpr int ROW = 192;                // bytes per 96-wide bf16 row
constexpr int SLAB = 32 * ROW;          // one 32-query slab of Q or dO

struct AttnP96 {
    const bf16_t* Q; const bf16_t* K; const bf16_t* V; bf16_t* O; float* LSE;
    const bf16_t* dO; bf16_t* dQ; bf16_t* dK; bf16_t* dV;
    const void* zero16;
    int64_t ldq, ldk, ldv, ldo;
    int B, heads, Sq, Sk;
    float scale; unsigned thr16; float inv_keep; unsigned key;
};

// stage rows [0, SP) of one head's [S][96] operand into a swizzled image by LDS-DMA (lane-linear destination: the permutation is
// on the source); rows >= nvalid read the zero page
__device__ __forceinline__ void stage_image96(char* img, const bf16_t* src, int64_t ld, int nvalid, const void* zero16, int w, int lane) {
    constexpr int NPC = SP * 12 / 64;
    static_assert(SP * 12 % 64 == 0, "image must be a whole number of 1-KiB pieces");
    for (int pc = w; pc < NPC; pc += NW) {
        const int P = pc * 64 + lane, r = P / 12, c = (P - r * 12) ^ swz<96>(r);
        glds16(r < nvalid ? (const void*)(src + (int64_t)r * ld + c * 8) : zero16, img + pc * 1024);
    }
}

// ================================================================================================ forward
__global__ __launch_bounds__(NT) void attn96_fwd_kernel(const AttnP96 p) {
    constexpr int QI = (NKT + NW - 1) / NW;          // query tiles per wave (ceil(Sq / 16) <= 18)
    extern __shared__ __attribute__((aligned(16))) char smem[];
    char* Ks = smem; char* Vs = smem + SP * ROW;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, g = lane >> 4, l15 = lane & 15;
    const int b = blockIdx.x / p.heads, h = blockIdx.x - b * p.heads;
    stage_image96(Ks, p.K + (int64_t)b * p.Sk * p.ldk + h * 96, p.ldk, p.Sk, p.zero16, w, lane);
    stage_image96(Vs, p.V + (int64_t)b * p.Sk * p.ldv + h * 96, p.ldv, p.Sk, p.zero16, w, lane);
    // the wave's query fragments, requested while the images fly (rows past Sq clamped: never stored)
    bf16x8 qf[QI][3];
#pragma unroll
    for (int it = 0; it < QI; ++it) {
        const int qc = min((w + NW * it) * 16 + l15, p.Sq - 1);
        const bf16_t* qrow = p.Q + ((int64_t)b * p.Sq + qc) * p.ldq + h * 96 + 8 * g;
#pragma unroll
        for (int i = 0; i < 3; ++i) qf[it][i] = *(const bf16x8*)(qrow + 32 * i);
    }
    // per-lane LDS offsets: chunk c ^ swz keeps c >> 2, so chunk groups 4i and 16-column tiles dt, dt + 2, dt + 4 are immediates
    const int kA = img_off<96>(l15, g), vT0 = tr_off<96>(g, l15, 0), vT1 = tr_off<96>(g, l15, 1);
    const AttDropLane dl = att_drop_lane(l15 & 3, true);
    const unsigned thrm1x2 = att_thrm1x2(p.thr16);
    const unsigned nQ4 = KZV_ATT_N4(p.Sq), nK4 = KZV_ATT_N4(p.Sk);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#pragma unroll
    for (int it = 0; it < QI; ++it)
#pragma unroll
        for (int i = 0; i < 3; ++i) pin(qf[it][i]);
    __syncthreads();

    const int nkt = (p.Sk + 15) >> 4, nqt = (p.Sq + 15) >> 4;
    const float sc = p.scale * LOG2E;
#pragma unroll
    for (int it = 0; it < QI; ++it) {
        const int qt = w + NW * it;
        if (qt >= nqt) break;
        const int q = qt * 16 + l15;
        // S^T tile: key on the accumulator rows (4g + r), query on the lane column
        f32x4 s[NKT];
        float mx = -INFINITY;
#pragma unroll
        for (int kt = 0; kt < NKT; ++kt) {
            s[kt] = (f32x4){0.f, 0.f, 0.f, 0.f};
            if (kt < nkt) {
#pragma unroll
                for (int i = 0; i < 3; ++i)
                    s[kt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(*(const bf16x8*)(Ks + kA + i * 64 + kt * 16 * ROW), qf[it][i], s[kt], 0, 0, 0);
                if (kt == nkt - 1) {                          // only the last tile can run past Sk
#pragma unroll
                    for (int r = 0; r < 4; ++r) s[kt][r] = kt * 16 + 4 * g + r < p.Sk ? s[kt][r] : -INFINITY;
                }
                mx = fmax3(mx, fmax3(s[kt][0], s[kt][1], s[kt][2]), s[kt][3]);
            }
        }
        mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
        mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
        const float mref = mx * sc;
        float sum = 0.f;
        unsigned pw[NKP * 4];                                 // bf16 pairs of the (dropped, un-normalised) probabilities
        const unsigned xw0 = att_block_word(b * p.heads + h, nQ4, (unsigned)q >> 2, nK4, g, p.key);
#pragma unroll
        for (int kt = 0; kt < NKT; ++kt) {
            if (kt < nkt) {
                att_fwd_tile(s[kt], sc, mref, sum, p.thr16, dl, xw0 + (unsigned)kt * (4u * KZV_ATT_GOLD), thrm1x2, pw + kt * 2);
            } else {
                pw[kt * 2] = 0u; pw[kt * 2 + 1] = 0u;
            }
        }
        sum += __shfl_xor(sum, 16, 64);
        sum += __shfl_xor(sum, 32, 64);
        if (p.LSE && g == 0 && q < p.Sq)
            p.LSE[((int64_t)b * p.heads + h) * p.Sq + q] = (mref + log2f(sum)) * (1.f / LOG2E);
        // O^T = V^T . P^T: 6 output tiles of 16 dimensions, 32 keys per step (V^T by transposed reads of the row-major image)
        f32x4 o[6];
#pragma unroll
        for (int dt = 0; dt < 6; ++dt) o[dt] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int kp = 0; kp < NKP; ++kp) {
            if (2 * kp < nkt) {
                const bf16x8 pf = words8(pw[kp * 4], pw[kp * 4 + 1], pw[kp * 4 + 2], pw[kp * 4 + 3]);
#pragma unroll
                for (int dt = 0; dt < 6; ++dt) {
                    const int t = ((dt & 1) ? vT1 : vT0) + (dt >> 1) * 64 + kp * 32 * ROW;
                    const bf16x8 vf = cat8(lds_tr16(Vs + t), lds_tr16(Vs + t + 16 * ROW));
                    o[dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vf, pf, o[dt], 0, 0, 0);
                }
            }
        }
        const float onorm = p.inv_keep / sum;
        if (q < p.Sq) {
            bf16_t* orow = p.O + ((int64_t)b * p.Sq + q) * p.ldo + h * 96 + 4 * g;
#pragma unroll
            for (int dt = 0; dt < 6; ++dt)
                store_bf4(orow + dt * 16, o[dt], onorm);
        }
    }
}

// =============================================================================================== backward
// LDS: K and V images (2 x 55,296 B), the Q / dO ring (2 x 2 x 6,144), dS^T [288 keys][32 queries] (18,432), LSE and delta rows
// (2 x 1,152): 155,904 B of the 163,840.
constexpr int BWD_LDS = 2 * SP * ROW + 4 * SLAB + SP * 64 + 2 * SP * 4;
static_assert(BWD_LDS <= 160 * 1024, "head_dim-96 attention backward must fit the LDS");

// one 32-query slab of Q and of dO: 768 16-byte chunks, two per thread (waves 4..7 repeat the last chunk for their second one: the
// loads stay unconditional).  Rows past the last query are CLAMPED to it: their LSE is +inf, so P = dS = 0 there.
__device__ __forceinline__ void slab_load(u32x4 v[2], const bf16_t* Qb, const bf16_t* dOb, int64_t ldq, int64_t ldo, int row0, int Sq, int tid) {
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int idx = min(tid + NT * j, 767), op = idx >= 384, i = idx - 384 * op;
        const int r = i / 12, c = i - r * 12, row = min(row0 + r, Sq - 1);
        const bf16_t* src = op ? dOb + (int64_t)row * ldo : Qb + (int64_t)row * ldq;
        v[j] = *(const u32x4*)(src + c * 8);
    }
}
__device__ __forceinline__ void slab_store(char* qs, char* os, const u32x4 v[2], int tid) {
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int idx = min(tid + NT * j, 767), op = idx >= 384, i = idx - 384 * op;
        const int r = i / 12, c = i - r * 12;
        *(u32x4*)((op ? os : qs) + img_off<96>(r, c)) = v[j];
    }
}

__global__ __launch_bounds__(NT) void attn96_bwd_kernel(const AttnP96 p) {
    constexpr int TPW = (NKT + NW - 1) / NW;                    // key tiles per wave
    static_assert(TPW <= 3, "dK/dV accumulators of more than 3 key tiles per wave do not fit the register file");
    extern __shared__ __attribute__((aligned(16))) char smem[];
    char* Ks = smem; char* Vs = Ks + SP * ROW;
    char* Qring = Vs + SP * ROW; char* Oring = Qring + 2 * SLAB;
    char* dST = Oring + 2 * SLAB;                               // [SP keys][32 queries] bf16, 8-byte units swizzled by key & 4
    float* lse = (float*)(dST + SP * 64);
    float* dlt = lse + SP;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, g = lane >> 4, l15 = lane & 15;
    const int b = blockIdx.x / p.heads, h = blockIdx.x - b * p.heads;
    const bf16_t* Qb = p.Q + (int64_t)b * p.Sq * p.ldq + h * 96;
    const bf16_t* dOb = p.dO + (int64_t)b * p.Sq * p.ldo + h * 96;
    const float keep_p = 1.f / p.inv_keep;
    // log-sum-exp (log2 units) and delta' = rowsum(dO . O) * P(keep) per query row: four lanes per row, 48 bytes each.  Loads
    // first, all at once; the image DMAs and the first slab go out behind them.
    constexpr int DR = (SP + NT / 4 - 1) / (NT / 4);
    bf16x8 ov[DR][3], dv8[DR][3];
    float lv[DR];
#pragma unroll
    for (int i = 0; i < DR; ++i) {
        const int row = min((tid >> 2) + i * (NT / 4), p.Sq - 1);
        const bf16_t* orow = p.O + ((int64_t)b * p.Sq + row) * p.ldo + h * 96 + (tid & 3) * 24;
        const bf16_t* drow = dOb + (int64_t)row * p.ldo + (tid & 3) * 24;
#pragma unroll
        for (int c = 0; c < 3; ++c) { ov[i][c] = *(const bf16x8*)(orow + 8 * c); dv8[i][c] = *(const bf16x8*)(drow + 8 * c); }
        lv[i] = p.LSE[((int64_t)b * p.heads + h) * p.Sq + row];
    }
    stage_image96(Ks, p.K + (int64_t)b * p.Sk * p.ldk + h * 96, p.ldk, p.Sk, p.zero16, w, lane);
    stage_image96(Vs, p.V + (int64_t)b * p.Sk * p.ldv + h * 96, p.ldv, p.Sk, p.zero16, w, lane);
    u32x4 sv[2];
    slab_load(sv, Qb, dOb, p.ldq, p.ldo, 0, p.Sq, tid);
    for (int i = tid; i < SP * 64 / 16; i += NT) ((uint4*)dST)[i] = make_uint4(0, 0, 0, 0);   // key rows no wave writes stay 0
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#pragma unroll
    for (int i = 0; i < DR; ++i) {
#pragma unroll
        for (int c = 0; c < 3; ++c) { pin(ov[i][c]); pin(dv8[i][c]); }
        pin(lv[i]);
    }
    pin(sv[0]); pin(sv[1]);
#pragma unroll
    for (int i = 0; i < DR; ++i) {
        const int row = (tid >> 2) + i * (NT / 4);
        float d = 0.f;
#pragma unroll
        for (int c = 0; c < 3; ++c) d = dot8(ov[i][c], dv8[i][c], d);
        d += __shfl_xor(d, 1, 64);      // att_row_stats written out: through the helper this kernel is allocated other registers
        d += __shfl_xor(d, 2, 64);
        if ((tid & 3) == 0 && row < SP) {
            lse[row] = row < p.Sq ? lv[i] * LOG2E : INFINITY;
            dlt[row] = row < p.Sq ? d * keep_p : 0.f;
        }
    }
    slab_store(Qring, Oring, sv, tid);
    __syncthreads();

    const int nkt = (p.Sk + 15) >> 4, nqb = (p.Sq + 31) >> 5;
    const float sc = p.scale * LOG2E;
    f32x4 dk[TPW][6], dv[TPW][6];
#pragma unroll
    for (int a = 0; a < TPW; ++a)
#pragma unroll
        for (int d = 0; d < 6; ++d) { dk[a][d] = (f32x4){0.f, 0.f, 0.f, 0.f}; dv[a][d] = (f32x4){0.f, 0.f, 0.f, 0.f}; }
    // per-lane LDS offsets: chunk c ^ swz keeps c >> 2, so chunk groups 4i and 16-column tiles dt, dt + 2, dt + 4 are immediates
    const int rA = img_off<96>(l15, g), tT0 = tr_off<96>(g, l15, 0), tT1 = tr_off<96>(g, l15, 1);
    const AttDropLane dl = att_drop_lane(l15 & 3, false);
    const int thr_s = att_thr_s(p.thr16);
    const unsigned nQ4 = KZV_ATT_N4(p.Sq), nK4 = KZV_ATT_N4(p.Sk);
    unsigned xslab = att_block_word(b * p.heads + h, nQ4, g, nK4, l15 >> 2, p.key);
    const unsigned xstep_t2 = 4u * nK4 * KZV_ATT_GOLD;
    // phase B: wave w takes the 16 queries t2 = w & 1 and the output tiles dt0 = w >> 1 and dt0 + 4 (the latter for dt0 < 2)
    const int bt2 = w & 1, dt0 = w >> 1;
    const int dsA = (4 * g + (l15 >> 2)) * 64 + (((bt2 * 4 + (l15 & 3)) ^ ((g & 1) << 2)) << 3);
    const int kT0 = tr_off<96>(g, l15, dt0), kT1 = tr_off<96>(g, l15, dt0 < 2 ? dt0 + 4 : dt0);

    for (int qb = 0; qb < nqb; ++qb) {
        const char* Qs = Qring + (qb & 1) * SLAB;
        const char* Os = Oring + (qb & 1) * SLAB;
        // ---------------- phase A: per owned key tile, S / dP / P / dS for 32 queries; dV^T, dK^T ----------
#pragma unroll
        for (int a = 0; a < TPW; ++a) {
            const int kt = w + NW * a;
            if (kt >= nkt) continue;
            const int key = kt * 16 + l15;
            char* dsrow = dST + key * 64;
            bf16x8 kf[3], vf[3];
#pragma unroll
            for (int i = 0; i < 3; ++i) { kf[i] = *(const bf16x8*)(Ks + rA + i * 64 + kt * 16 * ROW); vf[i] = *(const bf16x8*)(Vs + rA + i * 64 + kt * 16 * ROW); }
            // keys past Sk: -inf as the initial score accumulator (the key sits on the lane) makes their probabilities 0
            const float sinit = key < p.Sk ? 0.f : -INFINITY;
            unsigned pdw[4], dsw[4];
#pragma unroll
            for (int t2 = 0; t2 < 2; ++t2) {
                const f32x4 lq4 = *(const f32x4*)(lse + qb * 32 + t2 * 16 + 4 * g), dq4 = *(const f32x4*)(dlt + qb * 32 + t2 * 16 + 4 * g);
                f32x4 S = (f32x4){sinit, sinit, sinit, sinit}, dP = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int i = 0; i < 3; ++i) {
                    S = __builtin_amdgcn_mfma_f32_16x16x32_bf16(*(const bf16x8*)(Qs + rA + i * 64 + t2 * 16 * ROW), kf[i], S, 0, 0, 0);
                    dP = __builtin_amdgcn_mfma_f32_16x16x32_bf16(*(const bf16x8*)(Os + rA + i * 64 + t2 * 16 * ROW), vf[i], dP, 0, 0, 0);
                }
                unsigned u01 = 0, u23 = 0;
                if (p.thr16)      // block (q >> 2 = qb * 8 + t2 * 4 + g, key >> 2 = kt * 4 + (l15 >> 2)); this lane's column is key & 3
                    att_drop_u(dl, att_mix(xslab + (unsigned)t2 * xstep_t2 + (unsigned)kt * (4u * KZV_ATT_GOLD)), &u01, &u23);
                float pm[4], ds[4];
#pragma unroll
                for (int r = 0; r < 4; ++r) att_bwd_elem<false>(r, S[r], dP[r], sc, lq4[r], dq4[r], true, u01, u23, thr_s, pm[r], ds[r]);
                pdw[t2 * 2] = pack_bf2(pm[0], pm[1]); pdw[t2 * 2 + 1] = pack_bf2(pm[2], pm[3]);
                dsw[t2 * 2] = pack_bf2(ds[0], ds[1]); dsw[t2 * 2 + 1] = pack_bf2(ds[2], ds[3]);
                *(uint2*)(dsrow + (((t2 * 4 + g) ^ (key & 4)) << 3)) = make_uint2(dsw[t2 * 2], dsw[t2 * 2 + 1]);
            }
            const bf16x8 pf = words8(pdw[0], pdw[1], pdw[2], pdw[3]), df = words8(dsw[0], dsw[1], dsw[2], dsw[3]);
#pragma unroll
            for (int dt = 0; dt < 6; ++dt) {
                const int t = ((dt & 1) ? tT1 : tT0) + (dt >> 1) * 64;
                const bf16x8 dOt = cat8(lds_tr16(Os + t), lds_tr16(Os + t + 16 * ROW));
                const bf16x8 Qt = cat8(lds_tr16(Qs + t), lds_tr16(Qs + t + 16 * ROW));
                dv[a][dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(dOt, pf, dv[a][dt], 0, 0, 0);
                dk[a][dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(Qt, df, dk[a][dt], 0, 0, 0);
            }
        }
        __syncthreads();
        // the next slab (the last one again on the last block: the loads stay unconditional) flies during phase B; requested
        // during phase A, its 8 registers make the dK / dV accumulators spill
        slab_load(sv, Qb, dOb, p.ldq, p.ldo, min(qb + 1, nqb - 1) * 32, p.Sq, tid);
        // ---------------- phase B: dQ^T[d][q] = sum_key K^T[d][key] dS^T[key][q] for this 32-query slab ----
        {
            f32x4 acc0 = (f32x4){0.f, 0.f, 0.f, 0.f}, acc1 = acc0;
            const int nks = (nkt + 1) >> 1;
#pragma unroll
            for (int ks = 0; ks < NKP; ++ks) {
                if (ks < nks) {      // key slots: rows 32 ks + 4g + q, then the same 16 rows on
                    const bf16x8 dsf = cat8(lds_tr16(dST + dsA + ks * 2048), lds_tr16(dST + dsA + ks * 2048 + 1024));
                    const bf16x8 k0 = cat8(lds_tr16(Ks + kT0 + ks * 32 * ROW), lds_tr16(Ks + kT0 + ks * 32 * ROW + 16 * ROW));
                    acc0 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(k0, dsf, acc0, 0, 0, 0);
                    if (dt0 < 2) {
                        const bf16x8 k1 = cat8(lds_tr16(Ks + kT1 + ks * 32 * ROW), lds_tr16(Ks + kT1 + ks * 32 * ROW + 16 * ROW));
                        acc1 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(k1, dsf, acc1, 0, 0, 0);
                    }
                }
            }
            // the next slab has landed in registers: retired by hand before they are read, and before the dQ stores (vmcnt
            // retires in issue order: after them it would wait for the stores too)
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            pin(sv[0]); pin(sv[1]);
            const int q = qb * 32 + bt2 * 16 + l15;
            if (q < p.Sq) {
                const float osc = p.scale * p.inv_keep;
                bf16_t* row = p.dQ + ((int64_t)b * p.Sq + q) * p.ldq + h * 96 + 4 * g;
                store_bf4(row + dt0 * 16, acc0, osc);
                if (dt0 < 2)
                    store_bf4(row + (dt0 + 4) * 16, acc1, osc);
            }
            // the other ring buffer was last read in the previous block's phase A (two barriers ago)
            slab_store(Qring + ((qb + 1) & 1) * SLAB, Oring + ((qb + 1) & 1) * SLAB, sv, tid);
        }
        xslab += 2u * xstep_t2;
        __syncthreads();          // publishes the next slab and frees dS^T
    }
    const float ksc = p.scale * p.inv_keep;
#pragma unroll
    for (int a = 0; a < TPW; ++a) {
        const int key = (w + NW * a) * 16 + l15;
        if (w + NW * a >= nkt || key >= p.Sk) continue;
        bf16_t* krow = p.dK + ((int64_t)b * p.Sk + key) * p.ldk + h * 96 + 4 * g;
        bf16_t* vrow = p.dV + ((int64_t)b * p.Sk + key) * p.ldv + h * 96 + 4 * g;
#pragma unroll
        for (int dt = 0; dt < 6; ++dt) {
            store_bf4(krow + dt * 16, dk[a][dt], ksc);
            store_bf4(vrow + dt * 16, dv[a][dt], p.inv_keep);
        }
    }
}

constexpr int FWD_LDS = 2 * SP * ROW;

}  // namespace

// The launch: arguments were checked by kzv_attn_impl (attention_api.cpp), which sends head_dim 96, mode 0, Sq and Sk in 1..288 here.
int kzv_attn_d96(const kzv_attn_args* a, bool bwd, hipStream_t s) {
    AttnP96 p;
    kzv_attn_fill(p, a, 96);
    if (int rc = kzv_attn_fill_zero(p, "attn")) return rc;
    const int blocks = a->B * a->heads;
    if (!bwd) {
        kzv_launch_lds<attn96_fwd_kernel>(dim3(blocks), dim3(NT), FWD_LDS, s, p);
        return kzv_check_launch("attn_fwd (head_dim 96)");
    }
    kzv_launch_lds<attn96_bwd_kernel>(dim3(blocks), dim3(NT), BWD_LDS, s, p);
    return kzv_check_launch("attn_bwd (head_dim 96)");
}
