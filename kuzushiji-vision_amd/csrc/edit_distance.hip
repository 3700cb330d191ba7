// Levenshtein distance, edit counts, alignment and per-character error counts of (prediction row, label row) pairs of token ids:
//   kzv_edit_distance  over int64 id rows [n, ld] as generate* and the data loader produce them (include/kzv.h)
// What tokenizer.batch_decode(skip_special_tokens=True) x 2 + calculate_cer compute per line on the host, for a tokenizer of one character
// per token: the distance over the ids that are left once the specials are dropped IS the string distance.
// One wave per pair, four pairs per 256-thread workgroup (token_topk_kernel's launch shape); no workgroup barrier anywhere -- the four
// waves of a workgroup have different lengths and never wait for each other; a wave orders its own LDS traffic with wave_lds_sync.
//   1. compaction: a lane reads columns lane and lane + 64 of each row; an id stays if it lies in [0, vocab) and is none of the <= 8
//      special ids, wherever it stands (nothing is cut at the first EOS); ballot + popcount prefix give its place in LDS.  m = label
//      length, n = prediction length, both 0..128.
//   2. distance: Wagner-Fischer, unit costs, int32 -- the ROW-SCAN scheme (the one chosen; its disassembly holds no scratch).  Lane l owns
//      the two prediction columns j = 2l + 1, 2l + 2 of the current row in registers.  Per label row i:
//         T[j] = min(D[i-1][j] + 1, D[i-1][j-1] + (pred[j] != ref[i]))           (up, diagonal; one lane shift for the left neighbour)
//         D[i][j] = j + min over k <= j of (T[k] - k), T[0] = i                    (the run of insertions that ends in j)
//      the prefix minimum being a 6-step shuffle scan over the lanes' pair minima.  m rows, ~8 shuffles each.
//   3. alignment (only in the instance that has ops / an alignment / char_stats to write): 2 direction bits per cell, a lane keeps the
//      4 bits of its two cells for 8 rows in one register and stores one LDS word per 8 rows: 16 x 64 words = 4 KiB per wave.  THE RULE:
//      a cell's direction is DIAGONAL (match or substitution) if the diagonal attains the minimum, else UP (deletion of a label token),
//      else LEFT (insertion of a predicted token); along row 0 only left, along column 0 only up.  Lane 0 walks back from (m, n) and
//      writes the two index maps into LDS; then the whole wave classifies a label position and a prediction position per lane, counts
//      with ballots, stores the maps and adds to char_stats with integer atomics (the table is the same in every run).
// Every index is bounded by construction: compacted places < 128, ids that reach char_stats lie in [0, vocab), the walk takes at most
// m + n steps.  Plain HIP, vector stores only.
#include "kzv_common.h"
#include "../../include/kzv.h"
#include "kzv_host.h"

namespace {

constexpr int ED_MAX = 128;                                  // columns of a row, and so the longest compacted line
constexpr int DIR_DIAG = 0, DIR_UP = 1, DIR_LEFT = 2;

// orders this wave's LDS stores before its later LDS loads from other lanes (the LDS serves a wave's operations in order; this keeps
// the compiler from moving them across)
__device__ __forceinline__ void wave_lds_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// the ids of `row` that are neither special nor outside [0, vocab), in order, into out[0 .. count); returns count (wave-uniform)
__device__ __forceinline__ int compact_row(const int64_t* __restrict__ row, int width, const kzv_edit_args& a, int lane, int* out) {
    int count = 0;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int col = h * 64 + lane;
        const long long id = col < width ? (long long)row[col] : -1ll;
        bool keep = id >= 0 && id < (long long)a.vocab;
#pragma unroll
        for (int k = 0; k < 8; ++k)
            if (k < a.n_special && id == (long long)a.special[k]) keep = false;
        const unsigned long long mask = __ballot(keep);
        if (keep) out[count + __popcll(mask & ((1ull << lane) - 1ull))] = (int)id;
        count += __popcll(mask);
    }
    return __builtin_amdgcn_readfirstlane(count);
}

template <bool FULL>
__global__ __launch_bounds__(256) void edit_distance_kernel(const kzv_edit_args a) {
    __shared__ int s_tok[4][2][ED_MAX];                      // compacted label / prediction ids
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int pair = blockIdx.x * 4 + w;
    if (pair >= a.n) return;                                 // wave-uniform; no workgroup barrier follows
    int* const ref_tok = s_tok[w][0];
    int* const pred_tok = s_tok[w][1];
    const int m = compact_row(a.ref + (int64_t)pair * a.ld_ref, a.width_ref, a, lane, ref_tok);
    const int n = compact_row(a.pred + (int64_t)pair * a.ld_pred, a.width_pred, a, lane, pred_tok);
    wave_lds_sync();

    unsigned* dir = nullptr;                                 // [16][64]: word (i - 1) / 8 of lane l holds rows i of its two cells
    int* r2p = nullptr;
    int* p2r = nullptr;
    if constexpr (FULL) {
        __shared__ unsigned s_dir[4][ED_MAX / 8][64];
        __shared__ int s_map[4][2][ED_MAX];
        dir = &s_dir[w][0][0];
        r2p = s_map[w][0];
        p2r = s_map[w][1];
    }

    const int j0 = 2 * lane + 1, j1 = j0 + 1;               // this lane's columns; columns beyond n never feed a column <= n
    const int p0 = j0 <= n ? pred_tok[j0 - 1] : -1;
    const int p1 = j1 <= n ? pred_tok[j1 - 1] : -1;
    int d0 = j0, d1 = j1;                                    // row 0
    unsigned bits = 0;
    for (int i = 1; i <= m; ++i) {
        const int r = ref_tok[i - 1];                        // one address for the wave: a broadcast read
        int dl = __shfl_up(d1, 1, 64);                       // D[i-1][j0 - 1]
        if (lane == 0) dl = i - 1;
        const int dg0 = dl + (p0 != r ? 1 : 0), up0 = d0 + 1;
        const int dg1 = d0 + (p1 != r ? 1 : 0), up1 = d1 + 1;
        const int u0 = min(dg0, up0) - j0, u1 = min(dg1, up1) - j1;
        const int u01 = min(u0, u1);
        int s = lane == 0 ? min(u01, i) : u01;               // T[0] - 0 = i enters at lane 0
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int v = __shfl_up(s, o, 64);
            if (lane >= o) s = min(s, v);
        }
        int e = __shfl_up(s, 1, 64);                         // the minimum over every column left of this lane's
        if (lane == 0) e = i;
        const int n0 = j0 + min(e, u0), n1 = j1 + min(e, u01);
        if constexpr (FULL) {
            const unsigned c0 = n0 == dg0 ? DIR_DIAG : (n0 == up0 ? DIR_UP : DIR_LEFT);
            const unsigned c1 = n1 == dg1 ? DIR_DIAG : (n1 == up1 ? DIR_UP : DIR_LEFT);
            bits |= (c0 | (c1 << 2)) << (((i - 1) & 7) * 4);
            if ((i & 7) == 0 || i == m) { dir[((i - 1) >> 3) * 64 + lane] = bits; bits = 0; }
        }
        d0 = n0; d1 = n1;
    }
    int dist = m;                                            // n == 0: m deletions
    if (n > 0) dist = __shfl(((n - 1) & 1) ? d1 : d0, (n - 1) >> 1, 64);
    if (lane == 0) { a.dist[pair] = dist; a.ref_len[pair] = m; a.pred_len[pair] = n; }

    if constexpr (FULL) {
        r2p[lane] = -1; r2p[lane + 64] = -1;                 // a label token the walk does not pair is deleted,
        p2r[lane] = -1; p2r[lane + 64] = -1;                 // a predicted one inserted
        wave_lds_sync();
        if (lane == 0) {
            int i = m, j = n;
            for (int step = 0; step < 2 * ED_MAX && i > 0 && j > 0; ++step) {
                const unsigned code = (dir[((i - 1) >> 3) * 64 + ((j - 1) >> 1)] >> (((i - 1) & 7) * 4 + ((j - 1) & 1) * 2)) & 3u;
                if (code == DIR_DIAG) { r2p[i - 1] = j - 1; p2r[j - 1] = i - 1; --i; --j; }
                else if (code == DIR_UP) --i;
                else --j;
            }
        }
        wave_lds_sync();
        int n_cor = 0, n_sub = 0, n_del = 0, n_ins = 0;
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int x = h * 64 + lane;
            const bool in_ref = x < m, in_pred = x < n;
            const int to_pred = in_ref ? r2p[x] : -2, to_ref = in_pred ? p2r[x] : -2;
            const int rid = in_ref ? ref_tok[x] : 0, pid = in_pred ? pred_tok[x] : 0;
            const bool del = in_ref && to_pred < 0;
            const bool cor = in_ref && to_pred >= 0 && pred_tok[to_pred >= 0 ? to_pred : 0] == rid;
            const bool sub = in_ref && to_pred >= 0 && !cor;
            const bool ins = in_pred && to_ref < 0;
            n_cor += __popcll(__ballot(cor)); n_sub += __popcll(__ballot(sub));
            n_del += __popcll(__ballot(del)); n_ins += __popcll(__ballot(ins));
            if (a.ref_to_pred) {                             // both arrays or neither (checked by the launcher)
                if (x < a.width_ref) a.ref_to_pred[(int64_t)pair * a.ld_align + x] = to_pred;
                if (x < a.width_pred) a.pred_to_ref[(int64_t)pair * a.ld_align + x] = to_ref;
            }
            if (a.char_stats) {                              // rid, pid lie in [0, vocab): the compaction dropped everything else
                if (in_ref) {
                    int32_t* const row = a.char_stats + (int64_t)rid * 5;
                    atomicAdd(row + 0, 1);
                    atomicAdd(row + (cor ? 1 : (sub ? 2 : 3)), 1);
                }
                if (ins) atomicAdd(a.char_stats + (int64_t)pid * 5 + 4, 1);
            }
        }
        if (a.ops && lane < 4) a.ops[(int64_t)pair * 4 + lane] = lane == 0 ? n_cor : (lane == 1 ? n_sub : (lane == 2 ? n_del : n_ins));
    }
}

}  // namespace

extern "C" int kzv_edit_distance(const kzv_edit_args* a, void* stream) {
    if (!a) return kzv_fail(KZV_E_ARG, "edit_distance: null arguments");
    if (a->n < 0) return kzv_fail(KZV_E_ARG, "edit_distance: n must not be negative (got %d)", a->n);
    if (a->width_pred < 1 || a->width_pred > ED_MAX || a->width_ref < 1 || a->width_ref > ED_MAX)
        return kzv_fail(KZV_E_ARG, "edit_distance: widths must be in 1..%d (got width_pred %d, width_ref %d)", ED_MAX, a->width_pred, a->width_ref);
    if (a->ld_pred < a->width_pred || a->ld_ref < a->width_ref)
        return kzv_fail(KZV_E_ARG, "edit_distance: ld_pred %lld / ld_ref %lld smaller than the widths %d / %d", (long long)a->ld_pred,
                        (long long)a->ld_ref, a->width_pred, a->width_ref);
    if (a->n_special < 0 || a->n_special > 8) return kzv_fail(KZV_E_ARG, "edit_distance: n_special must be in 0..8 (got %d)", a->n_special);
    if (a->vocab < 1) return kzv_fail(KZV_E_ARG, "edit_distance: vocab must be positive (got %d)", a->vocab);
    if (!a->ref_to_pred != !a->pred_to_ref) return kzv_fail(KZV_E_ARG, "edit_distance: ref_to_pred and pred_to_ref come together or not at all");
    if (a->ref_to_pred && a->ld_align < (a->width_pred > a->width_ref ? a->width_pred : a->width_ref))
        return kzv_fail(KZV_E_ARG, "edit_distance: ld_align %lld smaller than the widths %d / %d", (long long)a->ld_align, a->width_pred, a->width_ref);
    if (a->n == 0) return KZV_OK;                            // nothing to do: nothing is launched, no array is looked at
    if (!a->pred || !a->ref) return kzv_fail(KZV_E_ARG, "edit_distance: null pred / ref rows");
    if (!a->dist || !a->ref_len || !a->pred_len) return kzv_fail(KZV_E_ARG, "edit_distance: null dist / ref_len / pred_len");
    const dim3 grid((unsigned)(((int64_t)a->n + 3) / 4)), block(256);
    if (a->ops || a->ref_to_pred || a->char_stats) hipLaunchKernelGGL(edit_distance_kernel<true>, grid, block, 0, (hipStream_t)stream, *a);
    else hipLaunchKernelGGL(edit_distance_kernel<false>, grid, block, 0, (hipStream_t)stream, *a);
    return kzv_check_launch("edit_distance");
}
