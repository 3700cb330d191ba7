// What the nodes of the score chain share (logits_process.hip, lm_fusion.hip, force_prefix.hip: one workgroup of 256 threads per row of
// one step's next-token scores): where a row's history or step lies, the row's log-sum-exp, and the host's checks of the arguments the
// three structs of include/kzv.h have in common (they share the field names, so everything here is templated on the struct).
#pragma once
#include "kzv_common.h"
#include "../../include/kzv.h"
#include "kzv_host.h"

constexpr int SCORE_MAX_VOCAB = 64 * 256;        // kzv_beam_topk's bound: a node's per-token bitmask is 2 KiB of LDS

// Row r's step index, its slot (lockstep: the row itself, or its group) and its image.  The three cases:
//   lockstep      slot_image == nullptr: t the host scalar
//   greedy slots  slot s = r (group 1): image slot_image[s] at slot_t[s]
//   beam slots    row r of slot s = r / group: image slot_image[s] at slot_t[s]
// with the step index of the slot cases read from device memory, so that one captured graph serves every step.
struct ScoreRow { int t, slot, image; int64_t hrow; };      // hrow: the row of ids that holds the row's history

// false: the row's slot is idle (slot_image < 0, or >= n_images) and the row stays as it is -- workgroup-uniform, so the caller returns
// before any barrier.  GROUPED: the lockstep rows come in groups as well (force_prefix, whose host check guarantees group >= 1).
// kzv_logits_process and kzv_lm_fuse never validate `group` in the lockstep case, where it may be 0: nothing divides by it there.
template <bool GROUPED, typename Args>
__device__ __forceinline__ bool score_row(const Args& p, int r, ScoreRow& o) {
    o.t = p.t;
    o.slot = o.image = GROUPED ? r / p.group : r;
    o.hrow = r;
    if (p.slot_image) {
        if (!GROUPED) o.slot = r / p.group;
        o.image = p.slot_image[o.slot];
        if (o.image < 0 || o.image >= p.n_images) return false;
        o.t = p.slot_t[o.slot];
        if (p.by_image) o.hrow = o.image;        // greedy slots: the wave's out_ids, a row per image
    }
    return true;
}

// The history h[0 .. n) of a located row, read where it lies
template <typename Args>
__device__ __forceinline__ const int64_t* score_history(const Args& p, const ScoreRow& o, int& n) {
    n = (int)min((int64_t)max(o.t + 1, 0), p.ld_ids);               // the history never leaves its row
    return p.ids + o.hrow * p.ld_ids;
}

// The maximum M and lse = log(sum exp(x - M)) of row[0 .. V), by the 256 threads of a workgroup, in the order of beam_topk_kernel's first
// phase (token_search.hip:168-199) -- the three agree bit for bit, which is what lets kzv_beam_rank_logprobs rank processed rows without
// a second normalisation: thread tid owns tokens tid + 256 e, loaded in batches of E independent loads; the WAVE's maximum first (wave_max
// of the threads' maxima), each thread's exponentials summed against it in ascending e, wave_sum, then the four waves' (max, sum) merged
// under the row maximum through s_m[4] / s_s[4].  It holds one barrier: every read of the row is done before the caller's first store.
// A MACRO, as KZV_DROP4 is: hipcc optimises a __forceinline__ function on its own before it inlines it, and the kernels then get another
// instruction stream than they had with the text in place (DESIGN 4m has what was tried).
#define KZV_ROW_MAX_LSE(E, row, V, tid, s_m, s_s, M, lse) do { \
    const int lane_ = (tid) & 63, w_ = (tid) >> 6; \
    float lm_ = -INFINITY; \
    for (int v0 = (tid); v0 < (V); v0 += 256 * (E)) { \
        float x[E]; \
        _Pragma("unroll") \
        for (int e = 0; e < (E); ++e) x[e] = (row)[min(v0 + e * 256, (V) - 1)]; \
        _Pragma("unroll") \
        for (int e = 0; e < (E); ++e) if (v0 + e * 256 < (V)) lm_ = fmaxf(lm_, x[e]); \
    } \
    const float wm_ = wave_max(lm_); \
    float ls_ = 0.f; \
    for (int v0 = (tid); v0 < (V); v0 += 256 * (E)) { \
        float x[E]; \
        _Pragma("unroll") \
        for (int e = 0; e < (E); ++e) x[e] = (row)[min(v0 + e * 256, (V) - 1)]; \
        _Pragma("unroll") \
        for (int e = 0; e < (E); ++e) ls_ += (v0 + e * 256 < (V) && x[e] != -INFINITY) ? expf(x[e] - wm_) : 0.f; \
    } \
    ls_ = wave_sum(ls_); \
    if (lane_ == 0) { (s_m)[w_] = wm_; (s_s)[w_] = ls_; } \
    __syncthreads(); \
    (M) = fmaxf(fmaxf((s_m)[0], (s_m)[1]), fmaxf((s_m)[2], (s_m)[3])); \
    float S_ = 0.f; \
    _Pragma("unroll") \
    for (int q = 0; q < 4; ++q) S_ += ((s_m)[q] == -INFINITY) ? 0.f : (s_s)[q] * expf((s_m)[q] - (M)); \
    (lse) = logf(S_); \
} while (0)

// What every entry refuses about the rows before any launch (KZV_E_ARG, `who` in the text).  HISTORY: the node reads token histories
// (ids, ld_ids) and its rows form groups in the slot cases only; else (force_prefix) the rows of an image form a group in every case.
template <bool HISTORY, typename Args>
static int score_rows_check(const Args* a, const char* who) {
    if constexpr (HISTORY) { if (!a->logits || !a->ids) return kzv_fail(KZV_E_ARG, "%s: null logits / ids", who); }
    else if (!a->logits) return kzv_fail(KZV_E_ARG, "%s: null logits", who);
    if (a->rows < 1) return kzv_fail(KZV_E_ARG, "%s: rows must be positive (got %d)", who, a->rows);
    if (a->vocab < 1 || a->vocab > SCORE_MAX_VOCAB) return kzv_fail(KZV_E_ARG, "%s: vocab %d outside 1..%d", who, a->vocab, SCORE_MAX_VOCAB);
    if (a->ld < a->vocab) return kzv_fail(KZV_E_ARG, "%s: ld %lld < vocab %d", who, (long long)a->ld, a->vocab);
    if constexpr (HISTORY) { if (a->ld_ids < 1) return kzv_fail(KZV_E_ARG, "%s: ld_ids must be positive", who); }
    if ((a->slot_image == nullptr) != (a->slot_t == nullptr)) return kzv_fail(KZV_E_ARG, "%s: slot_image and slot_t go together", who);
    if ((!HISTORY || a->slot_image) && (a->group < 1 || a->rows % a->group))
        return kzv_fail(KZV_E_ARG, "%s: %d rows are no multiple of %d rows per %s", who, a->rows, a->group, HISTORY ? "slot" : "image");
    if (a->slot_image && a->n_images < 1) return kzv_fail(KZV_E_ARG, "%s: n_images must be positive", who);
    if (!a->slot_image && a->t < 0) return kzv_fail(KZV_E_ARG, "%s: step %d is negative", who, a->t);
    return KZV_OK;
}
