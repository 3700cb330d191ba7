// N1: KV-cached decoder step: one new token per sequence attends over cached keys / values.
//
// Replaces, for generation only, the per-step work of HF RobertaSelfAttention / RobertaCrossAttention with `use_cache=True`
// (modeling_roberta.py:186-326) as driven by `decoder.generate` (src/models/trocr_model.py:306-316).  One wave per
// (sequence, head), fp32 scores and softmax in registers (see attn_decode_kernel); the self-attention variant also appends this
// step's key and value to the cache.  The reference's default 1024x64 columns give 256 cross-attention keys.
#include "kzv_common.h"
#include "../../include/kzv.h"
#include "kzv_host.h"
#include "kzv_kernels.h"

namespace {

struct DecAttnP {
    const bf16_t* q; int64_t ldq;                 // [B, ldq], head h at column h*64
    const bf16_t* knew; const bf16_t* vnew; int64_t ldnew;   // this step's key/value rows [B, ldnew] (self-attention) or null
    bf16_t* K; bf16_t* V; int64_t kb, kj, kh;     // key j, head h of sequence b: K + b*kb + h*kh + j*kj (same strides for V)
    const unsigned char* valid; int64_t ldvalid;  // [B, ldvalid]: key j usable (null: all)
    bf16_t* out; int64_t ldo;
    int nkeys, append_at, heads;                  // append_at >= 0: write knew/vnew at key index append_at first
    float scale;
    const int* tptr;                              // non-null: the step index t lives in device memory (graph replay): nkeys = t + 1, append_at = t
    int group;                                    // keys / values of sequence b live at batch index b / group (beams sharing one image's cross-attention K/V)
    int* rows; int64_t ldrows;                    // non-null (beam search): cached key j of sequence b lives in cache row rows[b * ldrows + j]
};

// One WAVE per (G sequences, head), no LDS and no barrier.  Every global access is a wave-instruction over 8 key (or value) rows x
// 128 contiguous bytes: lane = (row r = lane >> 3, 16-byte chunk c = lane & 7), iteration i owns key 8 i + r.  Scores: each
// lane multiplies its chunk of the key by the matching 8 query dimensions (registers), three shuffles sum the 8 chunks, so
// the 8 lanes of a row all hold that key's score; max and sum run across the wave.  Output: the SAME lanes hold the matching
// chunk of the value row, weight it by their key's probability, and three shuffles sum the 8 rows of an iteration.
// The step's own key / value (self-attention) is taken from the projection output directly and stored to the cache on the
// side.  NI = iterations (8 keys each): 24 -> 192 keys, 40 -> 320 keys.
// G > 1 (cross-attention of beam search): the G sequences of a wave are beams of ONE image and share its keys / values, which are
// loaded once and used for G queries (at one wave per beam the four beams re-read the same 41 KB through L2: 31.7 us per call
// at 1,024 rows against 23 us for the self-attention over a cache that does not fit the Infinity Cache).
template <int NI, int G>
__global__ __launch_bounds__(256) void attn_decode_kernel(const DecAttnP p, const int nunits) {
    const int unit = blockIdx.x * 4 + (threadIdx.x >> 6);          // (G sequences, head) of this wave
    if (unit >= nunits) return;
    const int b0 = (unit / p.heads) * G, h = unit - (unit / p.heads) * p.heads, lane = threadIdx.x & 63;
    const int b = b0;                                              // G == 1: the sequence
    bf16_t* Kb = p.K + (int64_t)(b0 / p.group) * p.kb + h * p.kh;
    bf16_t* Vb = p.V + (int64_t)(b0 / p.group) * p.kb + h * p.kh;
    const int tdev = p.tptr ? *p.tptr : 0;
    const int nkeys = p.tptr ? min(tdev + 1, 8 * NI) : p.nkeys;
    const int append_at = (G > 1) ? -1 : (p.tptr ? min(tdev, 8 * NI - 1) : p.append_at);
    const int r = lane >> 3, c = lane & 7;
    const bf16_t* knew = append_at >= 0 ? p.knew + (int64_t)b * p.ldnew + h * 64 : nullptr;
    const bf16_t* vnew = append_at >= 0 ? p.vnew + (int64_t)b * p.ldnew + h * 64 : nullptr;
    if (append_at >= 0) {                         // lane d copies dimension d of the new key and value into the cache
        Kb[(int64_t)append_at * p.kj + lane] = knew[lane];
        Vb[(int64_t)append_at * p.kj + lane] = vnew[lane];
        // ... and the row table learns where it went (own row): steps that are not followed by a re-parenting leave it complete.
        // No wave reads entry [b][append_at] during this step (that key comes from the projection output).
        if (G == 1 && p.rows && lane == 0 && h == 0) p.rows[(int64_t)b * p.ldrows + append_at] = b;
    }
    float qc[G][8];
#pragma unroll
    for (int g = 0; g < G; ++g) {
        const bf16x8 q8 = *(const bf16x8*)(p.q + (int64_t)(b0 + g) * p.ldq + h * 64 + c * 8);
#pragma unroll
        for (int e = 0; e < 8; ++e) qc[g][e] = bf2f((bf16_t)q8[e]) * p.scale;
    }
    // Beam search re-parents sequences every step; instead of copying cache rows (113 us per step at 1,024 rows), key j of
    // sequence b is read from the row of the ancestor that wrote it (rows[b][j], kzv_decode_reorder keeps the table).  This
    // step's own key is still stored to row b above and read from the projection output.
    int roff[G > 1 ? 1 : NI];                      // element offset of the ancestor's row relative to row b (checked < 2^31 on the host)
    if constexpr (G == 1) {
#pragma unroll
        for (int i = 0; i < NI; ++i) roff[i] = 0;
        if (p.rows) {                              // wave-uniform; the loads themselves are unconditional (clamped index) so that
            const int* tr = p.rows + (int64_t)b * p.ldrows;   // they all go out together instead of one round trip each
            int rj[NI];
#pragma unroll
            for (int i = 0; i < NI; ++i) rj[i] = tr[min(8 * i + r, (int)p.ldrows - 1)];
#pragma unroll
            for (int i = 0; i < NI; ++i) {
                const int j = 8 * i + r;
                roff[i] = (j < nkeys && j != append_at) ? (rj[i] - b) * (int)p.kb : 0;
            }
        }
    }
    auto row = [&](const bf16_t* base, const bf16_t* fresh, int i) -> bf16x8 {
        const int j = 8 * i + r;
        if (j >= nkeys) return (bf16x8){0, 0, 0, 0, 0, 0, 0, 0};
        return *(const bf16x8*)((j == append_at ? fresh : base + (G > 1 ? 0 : roff[G > 1 ? 0 : i]) + (int64_t)j * p.kj) + c * 8);
    };
    // key-usable flags of this lane's keys: loaded up front and unconditionally (clamped index) -- inside the score loop each one
    // sat in its own branch behind an s_waitcnt vmcnt(0), i.e. 24 serial round trips per self-attention call
    bool kok[G][NI];
#pragma unroll
    for (int g = 0; g < G; ++g)
#pragma unroll
        for (int i = 0; i < NI; ++i) kok[g][i] = true;
    if (p.valid) {
        unsigned char vb[G][NI];
#pragma unroll
        for (int g = 0; g < G; ++g)
#pragma unroll
            for (int i = 0; i < NI; ++i) vb[g][i] = p.valid[(int64_t)(b0 + g) * p.ldvalid + min(8 * i + r, (int)p.ldvalid - 1)];
#pragma unroll
        for (int g = 0; g < G; ++g)
#pragma unroll
            for (int i = 0; i < NI; ++i) kok[g][i] = vb[g][i] != 0;
    }
    float sc[G][NI];
    float mx[G];
#pragma unroll
    for (int g = 0; g < G; ++g) mx[g] = -INFINITY;
    // rows in flight: 8 wave-instructions = 64 keys.  (Requesting ALL key and value rows before the first score -- 225
    // registers -- changed nothing for 1,024 waves and cost the 4,096-wave beam step 6 ms per generation: occupancy.)
    constexpr int CH = 8;
#pragma unroll
    for (int i0 = 0; i0 < NI; i0 += CH) {
        if (i0 * 8 >= nkeys) {                     // wave-uniform: nothing left
#pragma unroll
            for (int g = 0; g < G; ++g)
#pragma unroll
                for (int u = 0; u < CH; ++u) sc[g][i0 + u] = -INFINITY;
            continue;
        }
        bf16x8 kk[CH];
#pragma unroll
        for (int u = 0; u < CH; ++u) kk[u] = row(Kb, knew, i0 + u);
#pragma unroll
        for (int u = 0; u < CH; ++u) {
            const int j = 8 * (i0 + u) + r;
            float kf[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) kf[e] = bf2f((bf16_t)kk[u][e]);
#pragma unroll
            for (int g = 0; g < G; ++g) {
                float a = 0.f;
#pragma unroll
                for (int e = 0; e < 8; ++e) a += qc[g][e] * kf[e];
                a += __shfl_xor(a, 1, 64); a += __shfl_xor(a, 2, 64); a += __shfl_xor(a, 4, 64);
                const bool ok = j < nkeys && kok[g][i0 + u];
                sc[g][i0 + u] = ok ? a : -INFINITY;
                mx[g] = fmaxf(mx[g], sc[g][i0 + u]);
            }
        }
    }
    float inv[G];
#pragma unroll
    for (int g = 0; g < G; ++g) {
        mx[g] = wave_max(mx[g]);
        const bool dead = mx[g] == -INFINITY;      // no usable key (a finished, all-pad row): output zeros
        float sum = 0.f;
#pragma unroll
        for (int i = 0; i < NI; ++i) { sc[g][i] = dead ? 0.f : __expf(sc[g][i] - mx[g]); sum += sc[g][i]; }
        sum = wave_sum(sum) * 0.125f;              // every key is counted by the 8 lanes of its row
        inv[g] = dead ? 0.f : 1.f / sum;
    }
    float o[G][8];
#pragma unroll
    for (int g = 0; g < G; ++g)
#pragma unroll
        for (int e = 0; e < 8; ++e) o[g][e] = 0.f;
#pragma unroll
    for (int i0 = 0; i0 < NI; i0 += CH) {
        if (i0 * 8 >= nkeys) continue;
        bf16x8 vv[CH];
#pragma unroll
        for (int u = 0; u < CH; ++u) vv[u] = row(Vb, vnew, i0 + u);
#pragma unroll
        for (int u = 0; u < CH; ++u) {
            float vf[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) vf[e] = bf2f((bf16_t)vv[u][e]);
#pragma unroll
            for (int g = 0; g < G; ++g)
#pragma unroll
                for (int e = 0; e < 8; ++e) o[g][e] += sc[g][i0 + u] * vf[e];
        }
    }
#pragma unroll
    for (int g = 0; g < G; ++g) {
#pragma unroll
        for (int e = 0; e < 8; ++e) { o[g][e] += __shfl_xor(o[g][e], 8, 64); o[g][e] += __shfl_xor(o[g][e], 16, 64); o[g][e] += __shfl_xor(o[g][e], 32, 64); }
        if (r == 0) {
            typedef __attribute__((ext_vector_type(4))) unsigned u32x4;
            const float iv = inv[g];
            const u32x4 pk = (u32x4){pack_bf2(o[g][0] * iv, o[g][1] * iv), pack_bf2(o[g][2] * iv, o[g][3] * iv), pack_bf2(o[g][4] * iv, o[g][5] * iv), pack_bf2(o[g][6] * iv, o[g][7] * iv)};
            *(u32x4*)(p.out + (int64_t)(b0 + g) * p.ldo + h * 64 + c * 8) = pk;
        }
    }
}

// Cross-attention keys / values for the generation steps: [layer][K|V][image][head][key][64] from the projection output
// [image * keys][layer][K|V][head][64] (one GEMM row per patch token).  There a head's key rows are 128-byte pieces 6 KB
// apart (17 us per call at 256 images: 2.5 TB/s); here each (image, head) streams one contiguous block.  Once per generation.
// The destination is a POOL of dst_images images ([layer][K|V][pool image][head][key][64]), written at entries first .. first + images - 1:
// slot-refill decoding keeps a whole wave's cross K/V resident (kzv_stream_encode); a plain generation has dst_images = images, first = 0.
__global__ __launch_bounds__(256) void cross_relayout_pool_kernel(const uint4* __restrict__ src, uint4* __restrict__ dst, int images, int keys, int heads,
                                                                  int layers2, int64_t total16, int dst_images, int first) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= total16) return;
    int64_t r = t;                                  // source-side order: [l2][img][h][key][8 chunks]
    const int c = r & 7; r >>= 3;
    const int key = r % keys; r /= keys;
    const int h = r % heads; r /= heads;
    const int img = r % images; r /= images;
    const int l2 = (int)r;
    dst[((((int64_t)l2 * dst_images + first + img) * heads + h) * keys + key) * 8 + c] = src[(((int64_t)img * keys + key) * layers2 + l2) * heads * 8 + h * 8 + c];
}

// beam re-parenting without moving the cache: dst[b][j] = src[parent[b]][j] for the keys written before this step, and the key
// the parent wrote at this step (index len - 1) sits in the parent's own row.  src == nullptr: the identity table (first step).
__global__ void kv_rows_kernel(const int* __restrict__ src, int* __restrict__ dst, const int64_t* __restrict__ parent, int B, int ld, int len) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= B * len) return;
    const int b = t / len, j = t - b * len;
    const int p = (int)parent[b];
    dst[(int64_t)b * ld + j] = (j == len - 1 || !src) ? p : src[(int64_t)p * ld + j];
}

// More than 320 keys (cross-attention over long encoder sequences; no cache append, no row table): the lane layout of
// attn_decode_kernel, but the keys are swept in chunks of 64 (8 wave-instructions of 8 rows) with a running max and sum per
// sequence, so nothing is held per key.  The output accumulators are rescaled when the max moves.
template <int G>
__global__ __launch_bounds__(256) void attn_decode_long_kernel(const DecAttnP p, const int nunits) {
    const int unit = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (unit >= nunits) return;
    const int b0 = (unit / p.heads) * G, h = unit - (unit / p.heads) * p.heads, lane = threadIdx.x & 63;
    const bf16_t* Kb = p.K + (int64_t)(b0 / p.group) * p.kb + h * p.kh;
    const bf16_t* Vb = p.V + (int64_t)(b0 / p.group) * p.kb + h * p.kh;
    const int nkeys = p.nkeys, r = lane >> 3, c = lane & 7;
    float qc[G][8];
#pragma unroll
    for (int g = 0; g < G; ++g) {
        const bf16x8 q8 = *(const bf16x8*)(p.q + (int64_t)(b0 + g) * p.ldq + h * 64 + c * 8);
#pragma unroll
        for (int e = 0; e < 8; ++e) qc[g][e] = bf2f((bf16_t)q8[e]) * p.scale;
    }
    constexpr int CH = 8;
    float mx[G], sum[G], o[G][8];
#pragma unroll
    for (int g = 0; g < G; ++g) {
        mx[g] = -INFINITY; sum[g] = 0.f;
#pragma unroll
        for (int e = 0; e < 8; ++e) o[g][e] = 0.f;
    }
    for (int j0 = 0; j0 < nkeys; j0 += 8 * CH) {
        bf16x8 kk[CH], vv[CH];
#pragma unroll
        for (int u = 0; u < CH; ++u) {
            const int j = min(j0 + 8 * u + r, nkeys - 1);          // clamped rows: their scores are masked below
            kk[u] = *(const bf16x8*)(Kb + (int64_t)j * p.kj + c * 8);
            vv[u] = *(const bf16x8*)(Vb + (int64_t)j * p.kj + c * 8);
        }
        bool kok[G][CH];
#pragma unroll
        for (int g = 0; g < G; ++g)
#pragma unroll
            for (int u = 0; u < CH; ++u) kok[g][u] = j0 + 8 * u + r < nkeys;
        if (p.valid) {
#pragma unroll
            for (int g = 0; g < G; ++g)
#pragma unroll
                for (int u = 0; u < CH; ++u)
                    kok[g][u] = kok[g][u] && p.valid[(int64_t)(b0 + g) * p.ldvalid + min(j0 + 8 * u + r, (int)p.ldvalid - 1)] != 0;
        }
        float sc[G][CH];
#pragma unroll
        for (int g = 0; g < G; ++g) {
            float cm = -INFINITY;
#pragma unroll
            for (int u = 0; u < CH; ++u) {
                float a = 0.f;
#pragma unroll
                for (int e = 0; e < 8; ++e) a += qc[g][e] * bf2f((bf16_t)kk[u][e]);
                a += __shfl_xor(a, 1, 64); a += __shfl_xor(a, 2, 64); a += __shfl_xor(a, 4, 64);
                sc[g][u] = kok[g][u] ? a : -INFINITY;
                cm = fmaxf(cm, sc[g][u]);
            }
            cm = wave_max(cm);
            const float mn = fmaxf(mx[g], cm);
            if (mn == -INFINITY) continue;                          // nothing usable yet (wave-uniform)
            const float alpha = __expf(mx[g] - mn);                 // 0 on the first usable chunk (mx = -inf)
            mx[g] = mn;
            sum[g] *= alpha;
#pragma unroll
            for (int e = 0; e < 8; ++e) o[g][e] *= alpha;
#pragma unroll
            for (int u = 0; u < CH; ++u) {
                const float pr = __expf(sc[g][u] - mn);
                sum[g] += pr;
#pragma unroll
                for (int e = 0; e < 8; ++e) o[g][e] += pr * bf2f((bf16_t)vv[u][e]);
            }
        }
    }
#pragma unroll
    for (int g = 0; g < G; ++g) {
        const bool dead = mx[g] == -INFINITY;                       // no usable key: output zeros
        const float iv = dead ? 0.f : 1.f / (wave_sum(sum[g]) * 0.125f);   // every key is counted by the 8 lanes of its row
#pragma unroll
        for (int e = 0; e < 8; ++e) { o[g][e] += __shfl_xor(o[g][e], 8, 64); o[g][e] += __shfl_xor(o[g][e], 16, 64); o[g][e] += __shfl_xor(o[g][e], 32, 64); }
        if (r == 0) {
            typedef __attribute__((ext_vector_type(4))) unsigned u32x4;
            const u32x4 pk = (u32x4){pack_bf2(o[g][0] * iv, o[g][1] * iv), pack_bf2(o[g][2] * iv, o[g][3] * iv), pack_bf2(o[g][4] * iv, o[g][5] * iv), pack_bf2(o[g][6] * iv, o[g][7] * iv)};
            *(u32x4*)(p.out + (int64_t)(b0 + g) * p.ldo + h * 64 + c * 8) = pk;
        }
    }
}

__global__ void step_inc_kernel(int* t) { *t += 1; }

}  // namespace

int kzv_step_inc(int* d_t, hipStream_t s) {
    hipLaunchKernelGGL(step_inc_kernel, dim3(1), dim3(1), 0, s, d_t);
    return kzv_check_launch("step_inc");
}

// tptr != nullptr: self-attention of graph-replayed step `*tptr` (nkeys = the cache capacity, which picks the kernel)
int kzv_attn_decode(const bf16_t* q, int64_t ldq, const bf16_t* knew, const bf16_t* vnew, int64_t ldnew, bf16_t* K, bf16_t* V, int64_t kb,
                    int64_t kj, const unsigned char* valid, int64_t ldvalid, bf16_t* out, int64_t ldo, int B, int heads, int nkeys,
                    int append_at, hipStream_t s, const int* tptr, int group, int* rows, int64_t ldrows, int64_t kh) {
    if (nkeys < 1 || nkeys > 4097) return kzv_fail(KZV_E_ARG, "attn_decode: 1..4097 keys");
    if (nkeys > 320 && (append_at >= 0 || tptr || rows)) return kzv_fail(KZV_E_ARG, "attn_decode: beyond 320 keys only without a cache append or row table");
    if (ldq % 8 || ldo % 8 || (knew && ldnew % 8)) return kzv_fail(KZV_E_ARG, "attn_decode: rows must be 16-byte aligned");
    if (group < 1 || (append_at >= 0 && group != 1)) return kzv_fail(KZV_E_ARG, "attn_decode: shared keys cannot be appended to");
    if (kj % 8) return kzv_fail(KZV_E_ARG, "attn_decode: key rows must be 16-byte aligned");
    if (rows && group != 1) return kzv_fail(KZV_E_ARG, "attn_decode: a row table and shared keys exclude each other");
    if (rows && (int64_t)B * kb >= (1ll << 31)) return kzv_fail(KZV_E_ARG, "attn_decode: cache too large for 32-bit row offsets");
    if (kh % 8) return kzv_fail(KZV_E_ARG, "attn_decode: head stride must be 16-byte aligned");
    DecAttnP p{q, ldq, knew, vnew, ldnew, K, V, kb, kj, kh, valid, ldvalid, out, ldo, nkeys, append_at, heads, 0.125f, tptr, group, rows, ldrows};
    // beams of one image (group > 1, shared keys): G of them per wave, G = the largest of 4, 3, 2 dividing the group
    const int G = group % 4 == 0 ? 4 : group % 3 == 0 ? 3 : group % 2 == 0 ? 2 : 1;
    const int nunits = (B / G) * heads;
#define KZV_AD(NI, GG) hipLaunchKernelGGL((attn_decode_kernel<NI, GG>), dim3((nunits + 3) / 4), dim3(256), 0, s, p, nunits)
#define KZV_AD_G(NI) do { if (G == 4) KZV_AD(NI, 4); else if (G == 3) KZV_AD(NI, 3); else if (G == 2) KZV_AD(NI, 2); else KZV_AD(NI, 1); } while (0)
#define KZV_ADL(GG) hipLaunchKernelGGL((attn_decode_long_kernel<GG>), dim3((nunits + 3) / 4), dim3(256), 0, s, p, nunits)
    if (nkeys <= 192) KZV_AD_G(24);
    else if (nkeys <= 320) KZV_AD_G(40);
    else if (G == 4) KZV_ADL(4); else if (G == 3) KZV_ADL(3); else if (G == 2) KZV_ADL(2); else KZV_ADL(1);
#undef KZV_ADL
#undef KZV_AD_G
#undef KZV_AD
    return kzv_check_launch("attn_decode");
}

int kzv_kv_rows(const int* src, int* dst, const int64_t* parent, int B, int ld, int len, hipStream_t s) {
    hipLaunchKernelGGL(kv_rows_kernel, dim3((B * len + 255) / 256), dim3(256), 0, s, src, dst, parent, B, ld, len);
    return kzv_check_launch("kv_rows");
}

int kzv_cross_relayout(const bf16_t* src, bf16_t* dst, int images, int keys, int heads, int layers2, hipStream_t s) {
    const int64_t total16 = (int64_t)layers2 * images * heads * keys * 8;
    hipLaunchKernelGGL(cross_relayout_pool_kernel, dim3((unsigned)((total16 + 255) / 256)), dim3(256), 0, s, (const uint4*)src, (uint4*)dst, images, keys, heads,
                       layers2, total16, images, 0);
    return kzv_check_launch("cross_relayout");
}

int kzv_cross_relayout_pool(const bf16_t* src, bf16_t* dst, int images, int keys, int heads, int layers2, int dst_images, int first, hipStream_t s) {
    if (images < 1 || first < 0 || first + images > dst_images) return kzv_fail(KZV_E_ARG, "cross_relayout_pool: entries %d .. %d outside a pool of %d images", first, first + images - 1, dst_images);
    const int64_t total16 = (int64_t)layers2 * images * heads * keys * 8;
    hipLaunchKernelGGL(cross_relayout_pool_kernel, dim3((unsigned)((total16 + 255) / 256)), dim3(256), 0, s, (const uint4*)src, (uint4*)dst, images, keys, heads,
                       layers2, total16, dst_images, first);
    return kzv_check_launch("cross_relayout_pool");
}
