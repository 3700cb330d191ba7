// Multi-head attention forward / backward for long sequences (Sq, Sk in 1..4,097), head_dim 64 and 96, no mask, bf16 MFMA.
//
// The whole-head kernels (attention.hip, attention_d96.hip) keep one head's K and V resident in LDS and stop at 288 keys.  These
// stream K / V through LDS instead (flash-style), so no buffer grows with Sq * Sk.  Same contract: kzv_attn_args, head h at column
// h * D, scale D^-0.5 in fp32, natural-log LSE [B, heads, Sq], the dropout masks of the packed 4 x 4-block generator of
// kzv_common.h with attention.hip's block index (b * heads + h, q >> 2, k >> 2); O / dQ / dK / dV are written, not accumulated.
// No device scratch, no atomics: every output element is produced by exactly one lane, so results are bitwise reproducible.
//
// The orientation is attention.hip's: S^T = K.Q^T with the KEY on the accumulator rows and the query on the lane column, the
// packed P^T accumulators are directly the B operand of O^T = V^T.P^T, and the softmax normalisation and 1 / P(keep) are applied
// to the outputs.
//   forward : a workgroup owns 128 queries of one (batch, head) (4 waves x 2 tiles of 16) and sweeps K / V in blocks of 64 keys,
//             double-buffered in LDS (LDS-DMA of the next block flies during the current one).  Online softmax: a running max and
//             a running sum per query row; the output accumulators are rescaled when the max moves.
//   backward: two kernels, both recomputing P from Q, K and the forward's LSE.
//             dK / dV: a workgroup owns 128 keys at head_dim 64, 64 at 96 (4 waves x 2 or 1 tiles of 16, K / V fragments in
//             registers) and sweeps the queries
//             in 32-query slabs of Q and dO through a 2-deep LDS ring, keeping dK^T / dV^T in registers; LSE and
//             delta' = rowsum(dO . O) * P(keep) of every query row are computed once into LDS first.
//             dQ: a workgroup owns 64 queries (a tile per wave) and sweeps K / V blocks like the forward; dS^T stays in
//             registers (query on the lane) and feeds dQ^T = K^T.dS^T directly.
// LDS images use the layout of the whole-head kernels (attention_common.h: swz / img_off / tr_off<D>), and their dropout
// bookkeeping and per-tile / per-element steps.  All LDS-DMA is issued from asm (glds16_asm): the waits are ours.
// The entry points (kzv_attn_stream_fwd / _bwd) and kzv_attn_stream_check are in attention_api.cpp.
#include "attention_common.h"

namespace {

constexpr int KB = 64;                  // keys per K / V block (forward, dQ)

struct StreamP {
    const bf16_t* Q; const bf16_t* K; const bf16_t* V; bf16_t* O; float* LSE;
    const bf16_t* dO; bf16_t* dQ; bf16_t* dK; bf16_t* dV;
    const void* zero16;
    int64_t ldq, ldk, ldv, ldo;
    int B, heads, Sq, Sk, nblk;          // nblk: query (forward, dQ) or key (dK / dV) blocks per (batch, head)
    float scale; unsigned thr16; float inv_keep; unsigned key;
};

// NR rows [row0, row0 + NR) of one head's [S][D] operand into a swizzled image by LDS-DMA (lane-linear destination, permuted
// source); rows >= nvalid read the zero page (zero != 0) or are clamped to the last row (zero == 0)
template <int D, int NR>
__device__ __forceinline__ void stage(char* img, const bf16_t* src, int64_t ld, int row0, int nvalid, const void* zero16, int w, int lane) {
    constexpr int CH = D / 8, NPC = NR * CH / 64;
    static_assert(NR * CH % 64 == 0, "image must be a whole number of 1-KiB pieces");
#pragma unroll
    for (int pc = w; pc < NPC; pc += 4) {
        const int P = pc * 64 + lane, r = P / CH, c = (P - r * CH) ^ swz<D>(r);
        const int row = row0 + r;
        const void* s = zero16 ? (row < nvalid ? (const void*)(src + (int64_t)row * ld + c * 8) : zero16)
                               : (const void*)(src + (int64_t)min(row, nvalid - 1) * ld + c * 8);
        glds16_asm(s, img + pc * 1024);
    }
}

__device__ __forceinline__ void lds_wait_barrier() {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
}

// ================================================================================================ forward
template <int D>
__global__ __launch_bounds__(256, 2) void stream_fwd_kernel(const StreamP p) {
    constexpr int ROW = 2 * D, NI = D / 32, NDT = D / 16, QT = 2, IMG = KB * ROW;
    extern __shared__ __attribute__((aligned(16))) char smem[];            // [2 buffers][K image, V image]
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, g = lane >> 4, l15 = lane & 15;
    const int bh = blockIdx.x / p.nblk, qblk = blockIdx.x - bh * p.nblk;
    const int b = bh / p.heads, h = bh - b * p.heads;
    const bf16_t* Kb = p.K + (int64_t)b * p.Sk * p.ldk + h * D;
    const bf16_t* Vb = p.V + (int64_t)b * p.Sk * p.ldv + h * D;
    const int nkb = (p.Sk + KB - 1) / KB, nqt = (p.Sq + 15) >> 4;
    stage<D, KB>(smem, Kb, p.ldk, 0, p.Sk, p.zero16, w, lane);
    stage<D, KB>(smem + IMG, Vb, p.ldv, 0, p.Sk, p.zero16, w, lane);
    bf16x8 qf[QT][NI];
#pragma unroll
    for (int it = 0; it < QT; ++it) {
        const int qc = min((qblk * 4 * QT + w * QT + it) * 16 + l15, p.Sq - 1);
        const bf16_t* qrow = p.Q + ((int64_t)b * p.Sq + qc) * p.ldq + h * D + 8 * g;
#pragma unroll
        for (int i = 0; i < NI; ++i) qf[it][i] = *(const bf16x8*)(qrow + 32 * i);
    }
    int kA[NI], vT[NDT];
#pragma unroll
    for (int i = 0; i < NI; ++i) kA[i] = img_off<D>(l15, 4 * i + g);
#pragma unroll
    for (int dt = 0; dt < NDT; ++dt) vT[dt] = tr_off<D>(g, l15, dt);
    AttDropLane dl = att_drop_lane(l15 & 3, true);
    const unsigned thrm1x2 = att_thrm1x2(p.thr16);
    const unsigned nQ4 = KZV_ATT_N4(p.Sq), nK4 = KZV_ATT_N4(p.Sk);
    unsigned xw0[QT];
#pragma unroll
    for (int it = 0; it < QT; ++it) {
        const int q = (qblk * 4 * QT + w * QT + it) * 16 + l15;
        xw0[it] = att_block_word(bh, nQ4, (unsigned)q >> 2, nK4, g, p.key);
    }
    const float sc = p.scale * LOG2E;
    float m[QT], l[QT];
    f32x4 o[QT][NDT];
#pragma unroll
    for (int it = 0; it < QT; ++it) {
        m[it] = -INFINITY; l[it] = 0.f;
#pragma unroll
        for (int dt = 0; dt < NDT; ++dt) o[it][dt] = (f32x4){0.f, 0.f, 0.f, 0.f};
    }
    lds_wait_barrier();
#pragma unroll
    for (int it = 0; it < QT; ++it)
#pragma unroll
        for (int i = 0; i < NI; ++i) pin(qf[it][i]);
    pin(dl);

    for (int kb = 0; kb < nkb; ++kb) {
        const char* Ks = smem + (kb & 1) * 2 * IMG;
        const char* Vs = Ks + IMG;
        if (kb + 1 < nkb) {
            char* nxt = smem + ((kb + 1) & 1) * 2 * IMG;
            stage<D, KB>(nxt, Kb, p.ldk, (kb + 1) * KB, p.Sk, p.zero16, w, lane);
            stage<D, KB>(nxt + IMG, Vb, p.ldv, (kb + 1) * KB, p.Sk, p.zero16, w, lane);
        }
        const bool last = kb == nkb - 1;
#pragma unroll
        for (int it = 0; it < QT; ++it) {
            if ((qblk * 4 * QT + w * QT + it) >= nqt) break;
            f32x4 s[4];
            float bm = -INFINITY;
#pragma unroll
            for (int kt = 0; kt < 4; ++kt) {
                s[kt] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int i = 0; i < NI; ++i)
                    s[kt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(*(const bf16x8*)(Ks + kA[i] + kt * 16 * ROW), qf[it][i], s[kt], 0, 0, 0);
                if (last) {                                   // only the last block can run past Sk
#pragma unroll
                    for (int r = 0; r < 4; ++r) s[kt][r] = kb * KB + kt * 16 + 4 * g + r < p.Sk ? s[kt][r] : -INFINITY;
                }
                bm = fmax3(bm, fmax3(s[kt][0], s[kt][1], s[kt][2]), s[kt][3]);
            }
            bm = fmaxf(bm, __shfl_xor(bm, 16, 64));
            bm = fmaxf(bm, __shfl_xor(bm, 32, 64));
            const float mn = fmaxf(m[it], bm);                // finite: every block holds a valid key
            const float alpha = __builtin_amdgcn_exp2f((m[it] - mn) * sc);
            m[it] = mn;
            l[it] *= alpha;
#pragma unroll
            for (int dt = 0; dt < NDT; ++dt) o[it][dt] *= alpha;
            const float mref = mn * sc;
            unsigned pw[8];                                   // bf16 pairs of the (dropped, un-normalised) probabilities
            const unsigned xw = xw0[it] + (unsigned)kb * (16u * KZV_ATT_GOLD);
#pragma unroll
            for (int kt = 0; kt < 4; ++kt) {
                float lsum = l[it];                           // a scalar local: see att_fwd_tile
                att_fwd_tile(s[kt], sc, mref, lsum, p.thr16, dl, xw + (unsigned)kt * (4u * KZV_ATT_GOLD), thrm1x2, pw + kt * 2);
                l[it] = lsum;
            }
#pragma unroll
            for (int kp = 0; kp < 2; ++kp) {
                const bf16x8 pf = words8(pw[kp * 4], pw[kp * 4 + 1], pw[kp * 4 + 2], pw[kp * 4 + 3]);
#pragma unroll
                for (int dt = 0; dt < NDT; ++dt) {
                    const int t = vT[dt] + kp * 32 * ROW;
                    const bf16x8 vf = cat8(lds_tr16(Vs + t), lds_tr16(Vs + t + 16 * ROW));
                    o[it][dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vf, pf, o[it][dt], 0, 0, 0);
                }
            }
        }
        lds_wait_barrier();        // the next block has landed; nobody reads this one any more
    }
#pragma unroll
    for (int it = 0; it < QT; ++it) {
        const int q = (qblk * 4 * QT + w * QT + it) * 16 + l15;
        float sum = l[it];
        sum += __shfl_xor(sum, 16, 64);
        sum += __shfl_xor(sum, 32, 64);
        if (q < p.Sq) {
            if (p.LSE && g == 0) p.LSE[(int64_t)bh * p.Sq + q] = (m[it] * sc + log2f(sum)) * (1.f / LOG2E);
            const float onorm = p.inv_keep / sum;
            bf16_t* orow = p.O + ((int64_t)b * p.Sq + q) * p.ldo + h * D + 4 * g;
#pragma unroll
            for (int dt = 0; dt < NDT; ++dt)
                store_bf4(orow + dt * 16, o[it][dt], onorm);
        }
    }
}

// ============================================================================================ backward dK / dV
// LDS: the Q / dO ring (2 x 2 x 32 rows) + LSE (log2 units) and delta' of every query row (ceil(Sq / 32) * 32 of each).
// Key tiles per wave: 2 at head_dim 64 (128 keys per workgroup); 1 at 96, where the dK / dV accumulators of two tiles spill.
template <int D> constexpr int kv_ring_bytes() { return 4 * 32 * 2 * D; }
template <int D> constexpr int kv_tiles() { return D == 64 ? 2 : 1; }

template <int D>
__global__ __launch_bounds__(256, 2) void stream_bwd_kv_kernel(const StreamP p) {
    constexpr int ROW = 2 * D, NI = D / 32, NDT = D / 16, KT = kv_tiles<D>(), SLAB = 32 * ROW;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, g = lane >> 4, l15 = lane & 15;
    const int bh = blockIdx.x / p.nblk, kblk = blockIdx.x - bh * p.nblk;
    const int b = bh / p.heads, h = bh - b * p.heads;
    const int nqs = (p.Sq + 31) >> 5, SqP = nqs * 32;
    float* lse = (float*)(smem + kv_ring_bytes<D>());
    float* dlt = lse + SqP;
    const bf16_t* Qb = p.Q + (int64_t)b * p.Sq * p.ldq + h * D;
    const bf16_t* dOb = p.dO + (int64_t)b * p.Sq * p.ldo + h * D;
    const bf16_t* Ob = p.O + (int64_t)b * p.Sq * p.ldo + h * D;
    const float keep_p = 1.f / p.inv_keep;
    stage<D, 32>(smem, Qb, p.ldq, 0, p.Sq, nullptr, w, lane);
    stage<D, 32>(smem + SLAB, dOb, p.ldo, 0, p.Sq, nullptr, w, lane);
    // this wave's key tiles: K / V row fragments (B operands of S = Q.K^T and dP = dO.V^T) straight from memory
    bf16x8 kf[KT][NI], vf[KT][NI];
#pragma unroll
    for (int a = 0; a < KT; ++a) {
        const int key = min((kblk * 4 * KT + w * KT + a) * 16 + l15, p.Sk - 1);
#pragma unroll
        for (int i = 0; i < NI; ++i) {
            kf[a][i] = *(const bf16x8*)(p.K + ((int64_t)b * p.Sk + key) * p.ldk + h * D + 32 * i + 8 * g);
            vf[a][i] = *(const bf16x8*)(p.V + ((int64_t)b * p.Sk + key) * p.ldv + h * D + 32 * i + 8 * g);
        }
    }
    // LSE and delta' of every query row: four lanes per row, D / 4 columns each, four rows per thread in flight
    for (int r0 = 0; r0 < SqP; r0 += 256) {
        float lv[4], dv[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int row = min(r0 + u * 64 + (tid >> 2), p.Sq - 1);
            const bf16_t* orow = Ob + (int64_t)row * p.ldo + (tid & 3) * (D / 4);
            const bf16_t* drow = dOb + (int64_t)row * p.ldo + (tid & 3) * (D / 4);
            float d = 0.f;
#pragma unroll
            for (int c = 0; c < D / 32; ++c) d += dot8(*(const bf16x8*)(orow + 8 * c), *(const bf16x8*)(drow + 8 * c));
            dv[u] = d;
            lv[u] = p.LSE[(int64_t)bh * p.Sq + row];
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) att_row_stats(dv[u], lv[u], keep_p, r0 + u * 64 + (tid >> 2), SqP, p.Sq, tid, lse, dlt);
    }
    const float sc = p.scale * LOG2E;
    f32x4 dk[KT][NDT], dvv[KT][NDT];
#pragma unroll
    for (int a = 0; a < KT; ++a)
#pragma unroll
        for (int d = 0; d < NDT; ++d) { dk[a][d] = (f32x4){0.f, 0.f, 0.f, 0.f}; dvv[a][d] = (f32x4){0.f, 0.f, 0.f, 0.f}; }
    int rA[NI], tT[NDT];
#pragma unroll
    for (int i = 0; i < NI; ++i) rA[i] = img_off<D>(l15, 4 * i + g);
#pragma unroll
    for (int dt = 0; dt < NDT; ++dt) tT[dt] = tr_off<D>(g, l15, dt);
    AttDropLane dl = att_drop_lane(l15 & 3, false);
    const int thr_s = att_thr_s(p.thr16);
    const unsigned nQ4 = KZV_ATT_N4(p.Sq), nK4 = KZV_ATT_N4(p.Sk);
    // pre-mix word of block (q >> 2 = g, k >> 2 = l15 >> 2) of slab 0, key tile 0; + per slab / 16-query half / key tile multiples of GOLD
    unsigned xslab = att_block_word(bh, nQ4, g, nK4, l15 >> 2, p.key);
    const unsigned xstep_t2 = 4u * nK4 * KZV_ATT_GOLD;
    lds_wait_barrier();
#pragma unroll
    for (int a = 0; a < KT; ++a)
#pragma unroll
        for (int i = 0; i < NI; ++i) { pin(kf[a][i]); pin(vf[a][i]); }
    pin(dl);

    for (int qs = 0; qs < nqs; ++qs) {
        const char* Qs = smem + (qs & 1) * 2 * SLAB;
        const char* Os = Qs + SLAB;
        if (qs + 1 < nqs) {
            char* nxt = smem + ((qs + 1) & 1) * 2 * SLAB;
            stage<D, 32>(nxt, Qb, p.ldq, (qs + 1) * 32, p.Sq, nullptr, w, lane);
            stage<D, 32>(nxt + SLAB, dOb, p.ldo, (qs + 1) * 32, p.Sq, nullptr, w, lane);
        }
        bf16x8 Qr[2][NI], Or[2][NI];
#pragma unroll
        for (int t2 = 0; t2 < 2; ++t2)
#pragma unroll
            for (int i = 0; i < NI; ++i) {
                Qr[t2][i] = *(const bf16x8*)(Qs + rA[i] + t2 * 16 * ROW);
                Or[t2][i] = *(const bf16x8*)(Os + rA[i] + t2 * 16 * ROW);
            }
#pragma unroll
        for (int a = 0; a < KT; ++a) {
            const int kt = kblk * 4 * KT + w * KT + a;
            const int key = kt * 16 + l15;
            if (kt * 16 >= p.Sk) break;
            // keys past Sk: -inf as the initial score accumulator (the key sits on the lane) makes their probabilities 0
            const float sinit = key < p.Sk ? 0.f : -INFINITY;
            unsigned pdw[4], dsw[4];
#pragma unroll
            for (int t2 = 0; t2 < 2; ++t2) {
                const f32x4 lq4 = *(const f32x4*)(lse + qs * 32 + t2 * 16 + 4 * g), dq4 = *(const f32x4*)(dlt + qs * 32 + t2 * 16 + 4 * g);
                f32x4 S = (f32x4){sinit, sinit, sinit, sinit}, dP = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int i = 0; i < NI; ++i) {
                    S = __builtin_amdgcn_mfma_f32_16x16x32_bf16(Qr[t2][i], kf[a][i], S, 0, 0, 0);
                    dP = __builtin_amdgcn_mfma_f32_16x16x32_bf16(Or[t2][i], vf[a][i], dP, 0, 0, 0);
                }
                unsigned u01 = 0, u23 = 0;
                if (p.thr16)      // block (q >> 2 = qs * 8 + t2 * 4 + g, key >> 2 = kt * 4 + (l15 >> 2)); this lane's column is key & 3
                    att_drop_u(dl, att_mix(xslab + (unsigned)t2 * xstep_t2 + (unsigned)kt * (4u * KZV_ATT_GOLD)), &u01, &u23);
                float pm[4], ds[4];
#pragma unroll
                for (int r = 0; r < 4; ++r) att_bwd_elem<false>(r, S[r], dP[r], sc, lq4[r], dq4[r], true, u01, u23, thr_s, pm[r], ds[r]);
                pdw[t2 * 2] = pack_bf2(pm[0], pm[1]); pdw[t2 * 2 + 1] = pack_bf2(pm[2], pm[3]);
                dsw[t2 * 2] = pack_bf2(ds[0], ds[1]); dsw[t2 * 2 + 1] = pack_bf2(ds[2], ds[3]);
            }
            const bf16x8 pf = words8(pdw[0], pdw[1], pdw[2], pdw[3]), df = words8(dsw[0], dsw[1], dsw[2], dsw[3]);
#pragma unroll
            for (int dt = 0; dt < NDT; ++dt) {
                const bf16x8 dOt = cat8(lds_tr16(Os + tT[dt]), lds_tr16(Os + tT[dt] + 16 * ROW));
                const bf16x8 Qt = cat8(lds_tr16(Qs + tT[dt]), lds_tr16(Qs + tT[dt] + 16 * ROW));
                dvv[a][dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(dOt, pf, dvv[a][dt], 0, 0, 0);
                dk[a][dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(Qt, df, dk[a][dt], 0, 0, 0);
            }
        }
        xslab += 2u * xstep_t2;
        lds_wait_barrier();        // the next slab has landed; nobody reads this one any more
    }
    const float ksc = p.scale * p.inv_keep;
#pragma unroll
    for (int a = 0; a < KT; ++a) {
        const int key = (kblk * 4 * KT + w * KT + a) * 16 + l15;
        if (key >= p.Sk) continue;
        bf16_t* krow = p.dK + ((int64_t)b * p.Sk + key) * p.ldk + h * D + 4 * g;
        bf16_t* vrow = p.dV + ((int64_t)b * p.Sk + key) * p.ldv + h * D + 4 * g;
#pragma unroll
        for (int dt = 0; dt < NDT; ++dt) {
            store_bf4(krow + dt * 16, dk[a][dt], ksc);
            store_bf4(vrow + dt * 16, dvv[a][dt], p.inv_keep);
        }
    }
}

// ================================================================================================ backward dQ
template <int D>
__global__ __launch_bounds__(256, 2) void stream_bwd_q_kernel(const StreamP p) {
    constexpr int ROW = 2 * D, NI = D / 32, NDT = D / 16, IMG = KB * ROW;
    extern __shared__ __attribute__((aligned(16))) char smem[];            // [2 buffers][K image, V image]
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, g = lane >> 4, l15 = lane & 15;
    const int bh = blockIdx.x / p.nblk, qblk = blockIdx.x - bh * p.nblk;
    const int b = bh / p.heads, h = bh - b * p.heads;
    const bf16_t* Kb = p.K + (int64_t)b * p.Sk * p.ldk + h * D;
    const bf16_t* Vb = p.V + (int64_t)b * p.Sk * p.ldv + h * D;
    const int nkb = (p.Sk + KB - 1) / KB;
    const int qt = qblk * 4 + w, q = qt * 16 + l15;
    const bool live = qt * 16 < p.Sq;                                       // wave-uniform
    stage<D, KB>(smem, Kb, p.ldk, 0, p.Sk, p.zero16, w, lane);
    stage<D, KB>(smem + IMG, Vb, p.ldv, 0, p.Sk, p.zero16, w, lane);
    // the query's rows (B operands: Q^T for S^T = K.Q^T, dO^T for dP^T = V.dO^T); delta' from dO and O, LSE (log2 units) per lane
    const int qc = min(q, p.Sq - 1);
    bf16x8 qf[NI], df[NI];
    float dpart = 0.f;
#pragma unroll
    for (int i = 0; i < NI; ++i) {
        qf[i] = *(const bf16x8*)(p.Q + ((int64_t)b * p.Sq + qc) * p.ldq + h * D + 32 * i + 8 * g);
        df[i] = *(const bf16x8*)(p.dO + ((int64_t)b * p.Sq + qc) * p.ldo + h * D + 32 * i + 8 * g);
        dpart += dot8(df[i], *(const bf16x8*)(p.O + ((int64_t)b * p.Sq + qc) * p.ldo + h * D + 32 * i + 8 * g));
    }
    dpart += __shfl_xor(dpart, 16, 64);
    dpart += __shfl_xor(dpart, 32, 64);
    float dq = dpart * (1.f / p.inv_keep);
    float lq = p.LSE[(int64_t)bh * p.Sq + qc] * LOG2E;
    int kA[NI], kT[NDT];
#pragma unroll
    for (int i = 0; i < NI; ++i) kA[i] = img_off<D>(l15, 4 * i + g);
#pragma unroll
    for (int dt = 0; dt < NDT; ++dt) kT[dt] = tr_off<D>(g, l15, dt);
    AttDropLane dl = att_drop_lane(l15 & 3, true);
    const int thr_s = att_thr_s(p.thr16);
    const unsigned nQ4 = KZV_ATT_N4(p.Sq), nK4 = KZV_ATT_N4(p.Sk);
    const unsigned xw0 = att_block_word(bh, nQ4, (unsigned)q >> 2, nK4, g, p.key);
    const float sc = p.scale * LOG2E;
    f32x4 acc[NDT];
#pragma unroll
    for (int dt = 0; dt < NDT; ++dt) acc[dt] = (f32x4){0.f, 0.f, 0.f, 0.f};
    lds_wait_barrier();
#pragma unroll
    for (int i = 0; i < NI; ++i) { pin(qf[i]); pin(df[i]); }
    pin(dq); pin(lq); pin(dl);

    for (int kb = 0; kb < nkb; ++kb) {
        const char* Ks = smem + (kb & 1) * 2 * IMG;
        const char* Vs = Ks + IMG;
        if (kb + 1 < nkb) {
            char* nxt = smem + ((kb + 1) & 1) * 2 * IMG;
            stage<D, KB>(nxt, Kb, p.ldk, (kb + 1) * KB, p.Sk, p.zero16, w, lane);
            stage<D, KB>(nxt + IMG, Vb, p.ldv, (kb + 1) * KB, p.Sk, p.zero16, w, lane);
        }
        if (live) {
            const bool last = kb == nkb - 1;
            unsigned dsw[8];
            const unsigned xw = xw0 + (unsigned)kb * (16u * KZV_ATT_GOLD);
#pragma unroll
            for (int kt = 0; kt < 4; ++kt) {
                f32x4 s = (f32x4){0.f, 0.f, 0.f, 0.f}, dp = s;
#pragma unroll
                for (int i = 0; i < NI; ++i) {
                    s = __builtin_amdgcn_mfma_f32_16x16x32_bf16(*(const bf16x8*)(Ks + kA[i] + kt * 16 * ROW), qf[i], s, 0, 0, 0);
                    dp = __builtin_amdgcn_mfma_f32_16x16x32_bf16(*(const bf16x8*)(Vs + kA[i] + kt * 16 * ROW), df[i], dp, 0, 0, 0);
                }
                unsigned u01 = 0, u23 = 0;
                if (p.thr16) att_drop_u(dl, att_mix(xw + (unsigned)kt * (4u * KZV_ATT_GOLD)), &u01, &u23);
                float ds[4];
#pragma unroll
                for (int r = 0; r < 4; ++r) {      // att_bwd_elem written out: its mask as an argument (!last || key < Sk) turns 15 selects into s_or
                    float pr = __builtin_amdgcn_exp2f(fmaf(s[r], sc, -lq));
                    if (last) pr = kb * KB + kt * 16 + 4 * g + r < p.Sk ? pr : 0.f;
                    const unsigned ur = (r & 2) ? u23 : u01;
                    const int us = (r & 1) ? (int)ur >> 16 : (int)(short)(ur & 0xffffu);
                    const float pm = us >= thr_s ? pr : 0.f;
                    ds[r] = fmaf(pm, dp[r], -pr * dq);
                }
                dsw[kt * 2] = pack_bf2(ds[0], ds[1]); dsw[kt * 2 + 1] = pack_bf2(ds[2], ds[3]);
            }
            // dQ^T[d][q] += K^T[d][key] dS^T[key][q], 32 keys per step (K^T by transposed reads of the row-major image)
#pragma unroll
            for (int kp = 0; kp < 2; ++kp) {
                const bf16x8 dsf = words8(dsw[kp * 4], dsw[kp * 4 + 1], dsw[kp * 4 + 2], dsw[kp * 4 + 3]);
#pragma unroll
                for (int dt = 0; dt < NDT; ++dt) {
                    const int t = kT[dt] + kp * 32 * ROW;
                    const bf16x8 kf = cat8(lds_tr16(Ks + t), lds_tr16(Ks + t + 16 * ROW));
                    acc[dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf, dsf, acc[dt], 0, 0, 0);
                }
            }
        }
        lds_wait_barrier();
    }
    if (q < p.Sq) {
        const float osc = p.scale * p.inv_keep;
        bf16_t* row = p.dQ + ((int64_t)b * p.Sq + q) * p.ldq + h * D + 4 * g;
#pragma unroll
        for (int dt = 0; dt < NDT; ++dt)
            store_bf4(row + dt * 16, acc[dt], osc);
    }
}

template <int D>
int run(const kzv_attn_args* a, bool bwd, hipStream_t s) {
    StreamP p;
    kzv_attn_fill(p, a, D);
    if (int rc = kzv_attn_fill_zero(p, "attn_stream")) return rc;
    const int bh = a->B * a->heads;
    constexpr int IMG2 = 2 * 2 * KB * 2 * D;                  // two buffers of a K and a V block
    constexpr int KV_MAX = kv_ring_bytes<D>() + 2 * ((KZV_ATTN_STREAM_MAX_S + 31) / 32 * 32) * 4;
    if (!bwd) {
        p.nblk = (a->Sq + 127) / 128;
        kzv_launch_lds<stream_fwd_kernel<D>>(dim3(bh * p.nblk), dim3(256), IMG2, s, p);
        return kzv_check_launch(D == 64 ? "attn_stream_fwd (head_dim 64)" : "attn_stream_fwd (head_dim 96)");
    }
    p.nblk = (a->Sk + 64 * kv_tiles<D>() - 1) / (64 * kv_tiles<D>());
    // the limit is raised to the most any launch of this kernel asks for (4,097 queries)
    kzv_launch_lds_max<stream_bwd_kv_kernel<D>>(dim3(bh * p.nblk), dim3(256), KV_MAX, kv_ring_bytes<D>() + 2 * ((a->Sq + 31) / 32 * 32) * 4, s, p);
    if (int rc = kzv_check_launch(D == 64 ? "attn_stream_bwd dK/dV (head_dim 64)" : "attn_stream_bwd dK/dV (head_dim 96)")) return rc;
    p.nblk = (a->Sq + 63) / 64;
    kzv_launch_lds<stream_bwd_q_kernel<D>>(dim3(bh * p.nblk), dim3(256), IMG2, s, p);
    return kzv_check_launch(D == 64 ? "attn_stream_bwd dQ (head_dim 64)" : "attn_stream_bwd dQ (head_dim 96)");
}

}  // namespace

// The launch: arguments were checked by kzv_attn_stream_check (attention_api.cpp); head_dim 96, else 64.
int kzv_attn_stream(const kzv_attn_args* a, bool bwd, hipStream_t s) {
    return a->head_dim == 96 ? run<96>(a, bwd, s) : run<64>(a, bwd, s);
}
