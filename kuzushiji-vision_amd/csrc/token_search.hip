// The token search of generation, i.e. what happens between two decoder steps (their attention: decode_attention.hip): greedy selection,
// beam ranking and update, and their slot-refill forms (kzv_stream_*, kzv_stream_beam_*).  Two rules carry every "stream equals static
// equals torch statement" test and are written once: the FIRST arg-max of a row (row_first_argmax) and the seating order (seat_rank).
#include "kzv_common.h"
#include "../../include/kzv.h"
#include "kzv_host.h"
#include "kzv_kernels.h"
#include "row_scan.h"
#include <cmath>
#include <initializer_list>

namespace {

// The first arg-max (value bv, column bi) of one fp32 logits row by 256 threads, in every thread: torch.argmax's, the smallest column
// among equal maxima.  Thread tid scans columns tid + 256 e in ascending order (strict >: its first), E per batch of independent loads
// (clamped index, masked afterwards); the wave's 64 candidates, then the 4 waves' (s_v / s_i [4], one barrier) merge under row_before.
template <int E>
__device__ __forceinline__ void row_first_argmax(const float* __restrict__ row, int V, int tid, float* s_v, int* s_i, float& bv, int& bi) {
    bv = -INFINITY; bi = ROW_NO_COL;
    for (int v0 = tid; v0 < V; v0 += 256 * E) {
        float x[E];
#pragma unroll
        for (int e = 0; e < E; ++e) x[e] = row[min(v0 + e * 256, V - 1)];
#pragma unroll
        for (int e = 0; e < E; ++e) { const int v = v0 + e * 256; if (v < V && x[e] > bv) { bv = x[e]; bi = v; } }
    }
    wave_first_argmax(bv, bi);
    if ((tid & 63) == 0) { s_v[tid >> 6] = bv; s_i[tid >> 6] = bi; }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < 4; ++q) if (row_before(s_v[q], s_i[q], bv, bi)) { bv = s_v[q]; bi = s_i[q]; }
}

// One pass of the seating prefix sum over 256 slots (thread tid holds one slot's ended flag): the ended slots BELOW this thread's within
// the pass, `total` = those of the whole pass.  Ballot + popcount per wave, s_w [4], one barrier; the caller's barrier frees s_w again.
__device__ __forceinline__ int seat_rank(bool ended, int tid, int* s_w, int& total) {
    const int lane = tid & 63, w = tid >> 6;
    const unsigned long long mask = __ballot(ended);
    if (lane == 0) s_w[w] = __popcll(mask);
    __syncthreads();
    int below = 0; total = 0;
#pragma unroll
    for (int q = 0; q < 4; ++q) { below += q < w ? s_w[q] : 0; total += s_w[q]; }
    return below + __popcll(mask & ((1ull << lane) - 1ull));
}

// the counters after a seating pass over all slots (one thread): next unseated image, lines / searches ended, steps taken
__device__ __forceinline__ void seat_counters(int* counters, int next, int ended_now, int n_images) {
    counters[0] = min(next + ended_now, n_images);
    const int ended = counters[1];
    counters[1] = ended + ended_now;
    if (ended < n_images) counters[2] += 1;      // steps issued past the end (the host looks only every few steps) do not count
}

// ---- slot-refill greedy decoding: selection and seating (kzv/stream.py::select_seat is the readable statement these are pinned against) ----
// A fixed set of decoder SLOTS (one workgroup of the one-launch step each) works through n_images images: slot b holds image
// slot_image[b] (< 0: idle) at step slot_t[b].  Per step, (1) stream_select_kernel, one workgroup per slot over its logits row: the first
// arg-max column (greedy_update_kernel's rule) and the row's log-sum-exp; the token goes to out_ids[image][t + 1], the line has ended on
// EOS or at its limit; (2) stream_seat_kernel, ONE workgroup over all slots: the slots whose lines ended take the next unseated images
// in ascending slot order (a prefix sum over the ended flags, no atomic ticket: the assignment is the same in every run), the others
// advance.  Nothing waits on another workgroup; the hand-off between the two is stream order.
struct StreamP {
    const float* logits; int64_t ld; int V;
    int slots, n_images, max_len, bos, eos, pad;
    int* slot_image; int* slot_t; int64_t* tokens; int* posids;     // [slots]
    int* counters;                                                  // next unseated image, lines ended, steps taken
    int* sel;                                                       // [slots][2]: ended, token (select -> seat)
    int64_t* out_ids; int64_t ld_ids; float* out_lp; int64_t ld_lp; const int* limit;
};

__global__ __launch_bounds__(256) void stream_select_kernel(const StreamP p) {
    __shared__ float s_v[4], s_s[4]; __shared__ int s_i[4];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int img = p.slot_image[b];
    if (img < 0) {                               // idle (workgroup-uniform, before any barrier)
        if (tid == 0) p.sel[2 * b] = 0;
        return;
    }
    const float* row = p.logits + (int64_t)b * p.ld;
    const int V = p.V; constexpr int E = 8;
    float bv; int bi;
    row_first_argmax<E>(row, V, tid, s_v, s_i, bv, bi);
    // log-sum-exp against the row maximum (the row is in cache): log p(token) = max - lse = -log(sum)
    float sum = 0.f;
    for (int v0 = tid; v0 < V; v0 += 256 * E) {
        float x[E];
#pragma unroll
        for (int e = 0; e < E; ++e) x[e] = row[min(v0 + e * 256, V - 1)];
#pragma unroll
        for (int e = 0; e < E; ++e) sum += (v0 + e * 256 < V) ? expf(x[e] - bv) : 0.f;
    }
    sum = wave_sum(sum);
    if (lane == 0) s_s[w] = sum;
    __syncthreads();
    if (tid == 0) {
        sum = (s_s[0] + s_s[1]) + (s_s[2] + s_s[3]);
        const int t = p.slot_t[b];
        int lim = p.limit ? min(p.limit[img], p.max_len) : p.max_len;
        if (t + 1 < p.max_len && img < p.n_images) {
            p.out_ids[(int64_t)img * p.ld_ids + t + 1] = bi;
            if (p.out_lp) p.out_lp[(int64_t)img * p.ld_lp + t + 1] = -logf(sum);
        }
        p.sel[2 * b] = (bi == p.eos || t + 2 >= lim) ? 1 : 0;
        p.sel[2 * b + 1] = bi;
    }
}

// a slot at the start of a line: step 0, BOS, the first RoBERTa position
__device__ __forceinline__ void stream_reset(const StreamP& p, int s) { p.slot_t[s] = 0; p.tokens[s] = p.bos; p.posids[s] = p.pad + 1; }

__global__ __launch_bounds__(256) void stream_seat_kernel(const StreamP p) {
    __shared__ int s_w[4];
    const int tid = threadIdx.x, next = p.counters[0];
    int carry = 0;                               // lines ended in the slots below this pass
    for (int base = 0; base < p.slots; base += 256) {
        const int s = base + tid;
        const bool in = s < p.slots;
        const int e = in ? p.sel[2 * s] : 0;
        int total;
        const int rank = carry + seat_rank(e != 0, tid, s_w, total);      // ended slots below slot s
        if (in) {
            if (e) {
                const int ni = next + rank;
                p.slot_image[s] = ni < p.n_images ? ni : -1;
                stream_reset(p, s);
            } else if (p.slot_image[s] >= 0) {
                const int t = p.slot_t[s];
                p.slot_t[s] = t + 1; p.tokens[s] = p.sel[2 * s + 1]; p.posids[s] = t + 2 + p.pad;
            }
        }
        carry += total;
        __syncthreads();
    }
    if (tid == 0) seat_counters(p.counters, next, carry, p.n_images);
}

// the first min(slots, n_images) images take the slots in order; the other slots are idle
__global__ void stream_start_kernel(const StreamP p) {
    const int s = blockIdx.x * 256 + threadIdx.x;
    if (s < p.slots) {
        p.slot_image[s] = s < p.n_images ? s : -1;
        stream_reset(p, s);
    }
    if (s == 0) { p.counters[0] = min(p.slots, p.n_images); p.counters[1] = 0; p.counters[2] = 0; }
}

// One beam-search step's ranking for one image (HF GenerationMixin._get_top_k_continuations, transformers generation/utils.py:
// log_softmax of each beam's next-token logits + the beam's accumulated score, then the K best of the nb * V continuations in
// descending order; equal scores rank by the smaller flat index beam * V + token).  One workgroup per image.  Every thread
// owns E = ceil(V / 256) tokens of each beam row and reads them as ONE batch of independent loads (a scalar loop here exposed a
// memory round trip per element: 58 us per launch): first for the row's (max, sum of exponentials), combined across the
// workgroup; then (cache hits) for the candidates, kept as a sorted top-KM list per thread in registers.  Each wave then
// extracts its K best by shuffles, and one wave merges the four lists.
// Replaces torch's log_softmax + two radix-select top-k passes + gathers (~190 us per step at 256 images) by one launch.
struct Cand { float v; int i; };
__device__ __forceinline__ bool cand_better(float av, int ai, float bv, int bi) { return av > bv || (av == bv && ai < bi); }

// LSE = false (kzv_beam_rank_logprobs): the rows already hold log-probabilities (kzv_logits_process has normalised and processed them; a
// banned token is -inf and never enters a list), so the log-sum-exp phase is compiled out and a continuation is x + beam score.
template <int KM, int E, bool LSE = true>
__global__ __launch_bounds__(256) void beam_topk_kernel(const float* __restrict__ logits, int64_t ld, const float* __restrict__ run_sc, int nb, int V, int K,
                                                        float* __restrict__ out_lp, int64_t* __restrict__ out_ix) {
    constexpr int NBM = 8;
    __shared__ float s_m[4][NBM], s_s[4][NBM];
    __shared__ float s_cv[4][16]; __shared__ int s_ci[4][16];
    const int img = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const float* base = logits + (int64_t)img * nb * ld;
    // ---- per-row log-sum-exp: local (max, sum) over this thread's E tokens, then across the workgroup ----
    float lm[NBM], ls[NBM];
    float rmx[NBM], rlse[NBM];
    if constexpr (LSE) {
#pragma unroll
    for (int k = 0; k < NBM; ++k) {
        lm[k] = -INFINITY; ls[k] = 0.f;
        if (k < nb) {
            float x[E];
#pragma unroll
            for (int e = 0; e < E; ++e) { const int v = tid + e * 256; x[e] = base[(int64_t)k * ld + min(v, V - 1)]; if (v >= V) x[e] = -INFINITY; }
#pragma unroll
            for (int e = 0; e < E; ++e) lm[k] = fmaxf(lm[k], x[e]);
            const float wm = wave_max(lm[k]);          // finite: every row has V >= 1 real entries somewhere in the wave? not per wave:
            lm[k] = wm;                                // a wave past the end of a short row holds -inf and contributes exp(-inf) = 0 below
#pragma unroll
            for (int e = 0; e < E; ++e) ls[k] += (x[e] == -INFINITY) ? 0.f : expf(x[e] - wm);
            ls[k] = wave_sum(ls[k]);
        }
    }
    if (lane == 0)
#pragma unroll
        for (int k = 0; k < NBM; ++k) { s_m[w][k] = lm[k]; s_s[w][k] = ls[k]; }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < NBM; ++k) {
        const float M = fmaxf(fmaxf(s_m[0][k], s_m[1][k]), fmaxf(s_m[2][k], s_m[3][k]));
        float S = 0.f;
#pragma unroll
        for (int q = 0; q < 4; ++q) S += (s_m[q][k] == -INFINITY) ? 0.f : s_s[q][k] * expf(s_m[q][k] - M);
        rmx[k] = M; rlse[k] = logf(S);
    }
    }                                            // if constexpr (LSE): the block keeps its former indentation
    // ---- this thread's best KM continuations, best first (flat indices arrive in increasing order: ties keep the smaller) ----
    float tv[KM]; int ti[KM];
#pragma unroll
    for (int q = 0; q < KM; ++q) { tv[q] = -INFINITY; ti[q] = 0x7fffffff; }
#pragma unroll
    for (int k = 0; k < NBM; ++k) {
        if (k < nb) {
            const float sc = run_sc[img * nb + k];
            float x[E];
#pragma unroll
            for (int e = 0; e < E; ++e) x[e] = base[(int64_t)k * ld + min(tid + e * 256, V - 1)];
#pragma unroll
            for (int e = 0; e < E; ++e) {
                const int v = tid + e * 256;
                const float val = LSE ? ((x[e] - rmx[k]) - rlse[k]) + sc : x[e] + sc;
                if (v < V && val > tv[KM - 1]) {
                    tv[KM - 1] = val; ti[KM - 1] = k * V + v;
#pragma unroll
                    for (int q = KM - 1; q > 0; --q)
                        if (tv[q] > tv[q - 1]) { const float a = tv[q]; tv[q] = tv[q - 1]; tv[q - 1] = a; const int b = ti[q]; ti[q] = ti[q - 1]; ti[q - 1] = b; }
                }
            }
        }
    }
    // ---- each wave extracts its K best (no barrier), then wave 0 merges the 4 x K ----
    for (int r = 0; r < K; ++r) {
        float bv = tv[0]; int bi = ti[0]; int bl = lane;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const float ov = __shfl_xor(bv, o, 64); const int oi = __shfl_xor(bi, o, 64); const int ol = __shfl_xor(bl, o, 64);
            if (cand_better(ov, oi, bv, bi)) { bv = ov; bi = oi; bl = ol; }
        }
        if (lane == 0) { s_cv[w][r] = bv; s_ci[w][r] = bi; }
        if (lane == bl) {
#pragma unroll
            for (int q = 0; q + 1 < KM; ++q) { tv[q] = tv[q + 1]; ti[q] = ti[q + 1]; }
            tv[KM - 1] = -INFINITY; ti[KM - 1] = 0x7fffffff;
        }
    }
    __syncthreads();
    if (w == 0) {
        float cv = -INFINITY; int ci = 0x7fffffff;                 // lane = list (lane >> 4) entry (lane & 15)
        if ((lane & 15) < K) { cv = s_cv[lane >> 4][lane & 15]; ci = s_ci[lane >> 4][lane & 15]; }
        for (int r = 0; r < K; ++r) {
            float bv = cv; int bi = ci; int bl = lane;
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {
                const float ov = __shfl_xor(bv, o, 64); const int oi = __shfl_xor(bi, o, 64); const int ol = __shfl_xor(bl, o, 64);
                if (cand_better(ov, oi, bv, bi)) { bv = ov; bi = oi; bl = ol; }
            }
            // (fewer than K continuations above -inf, possible under a mask only: the empty entries come out as -inf at index 0, inside the tables)
            if (!LSE && bi == 0x7fffffff) bi = 0;
            if (lane == 0) { out_lp[(int64_t)img * K + r] = bv; out_ix[(int64_t)img * K + r] = bi; }
            if (lane == bl) { cv = -INFINITY; ci = 0x7fffffff; }
        }
    }
}

// One beam-search step's bookkeeping for one image: what kzv/beam.py::beam_search does between two decoder steps with ~35 small
// torch kernels (~270 us per step), restated from transformers' GenerationMixin._beam_search (generation/utils.py:3208-3508:
// _get_running_beams_for_next_iteration, _update_finished_beams, _check_early_stop_heuristic) -- kzv/beam.py is the readable
// statement and the CPU path pinned against HF; this kernel is checked against it state for state (tests/test_ops_gpu.py).
// One wave per image: lane 0 does the scalar ranking (K <= 16 continuations, nb <= 8 beams), all lanes copy token rows.
struct BeamUpd {
    const float* top_lp; const int64_t* top_ix;                   // [B, K] from kzv_beam_topk
    const int64_t* run_seq_in; int64_t* run_seq_out;              // [B, nb, L]
    const int64_t* fin_seq_in; int64_t* fin_seq_out;              // [B, nb, L]
    float* run_sc; float* fin_sc; unsigned char* fin_done; int64_t* fin_len; unsigned char* unsat;   // [B, nb] / [B]
    int64_t* rows;                                                // [B * nb]: former flat row each running beam continues from
    int* flags;                                                   // [5]: images still unsatisfied, images whose finished list is not full, images with a continuation that did not stop; [3] = stopped, [4] = updates applied
    int nb, K, L, V, cur, eos, early;
    float div;                                                    // cur ** length_penalty as fp32: the length divisor of a hypothesis that ends at this step
    const float* run_lp_in; float* run_lp_out;                    // [B, nb, L] fp32 or null: the token rows' per-token log-probabilities (LP instance)
    const float* fin_lp_in; float* fin_lp_out;
    const int* prefix_len; const float* divtab;                   // PFX instance: [B] prefix lengths, [L + 1] fp32 of n ** length_penalty
};

// One image's step, ranked: what one lane works out between the loads and the row copies.  The inputs are filled by the lanes together
// (read by one lane alone they were as many serial round trips); the outputs are read by all of them.  Shared by beam_update_kernel
// (every image at the launch's cur) and stream_beam_update_kernel (every slot at its own).
struct BeamRank {
    float lp[16]; int64_t ix[16];                                // in: the K ranked continuations
    float fsc[8]; int64_t flen[8]; unsigned char fdone[8]; unsigned char unsat;      // in: the finished list, the image's unsatisfied flag
    int src[16], tok[16]; unsigned char hit[16];                 // out: per continuation
    int nxt[8], mix[8];                                          // out: continuation of running beam i; merged-list entry of finished row i (< nb: an old row)
};
struct BeamRankOut {                                             // the ranking lane's own copy of what it stores afterwards
    float run_new[8], fsc_new[8]; int64_t fl_new[8]; unsigned char fd_new[8];
    bool un, done_new, all_hits;                                 // still unsatisfied, finished list full, every continuation stopped
};

// the co-operative fill from row b (an image, or a slot) of the ranking [.., K] and of the finished state [.., nb]: one load per thread, together
__device__ __forceinline__ void beam_rank_load(BeamRank& r, int tid, int K, int nb, int b, const float* lp, const int64_t* ix, const float* fsc,
                                               const unsigned char* fdone, const int64_t* flen, const unsigned char* unsat) {
    if (tid < K) { r.lp[tid] = lp[(int64_t)b * K + tid]; r.ix[tid] = ix[(int64_t)b * K + tid]; }
    if (tid >= 16 && tid < 16 + nb) { const int i = tid - 16; r.fsc[i] = fsc[b * nb + i]; r.fdone[i] = fdone[b * nb + i]; r.flen[i] = flen[b * nb + i]; }
    if (tid == 32) r.unsat = unsat[b];
}

// `lim`: the length at which a continuation stops whatever its token (max_len, or the image's own limit); `div`: the length divisor at cur
__device__ __forceinline__ void beam_rank(BeamRank& r, BeamRankOut& o, int nb, int K, int V, int eos, int cur, int lim, int early, float div) {
    constexpr float NEG = -1.0e9f;
    float s2[16], msc[24];
    unsigned char mdone[24];
    bool all_hits = true, all_done = true;
    for (int i = 0; i < nb; ++i) all_done = all_done && r.fdone[i];
    const float full_neg = (all_done && early) ? NEG : 0.f;
    const float unsat_neg = r.unsat ? 0.f : NEG;
    for (int k = 0; k < K; ++k) {
        const int64_t ix = r.ix[k];
        const float lp = r.lp[k];
        const int src = min((int)(ix / V), nb - 1), tok = (int)min(ix - (int64_t)src * V, (int64_t)V - 1);     // in range whatever a row of NaN logits ranked
        const bool hit = tok == eos || cur + 1 >= lim;
        r.src[k] = src; r.tok[k] = tok; r.hit[k] = hit;
        all_hits = all_hits && hit;
        s2[k] = lp + (hit ? NEG : 0.f);
        const bool just = hit && k < nb;
        float f = lp / div;
        f = f + full_neg; f = f + unsat_neg; f = f + (just ? 0.f : NEG);
        msc[nb + k] = f; mdone[nb + k] = just;
    }
    // running beams of the next step: the best nb continuations that did not stop (equal scores: the smaller rank first)
    unsigned used = 0;
    for (int i = 0; i < nb; ++i) {
        int best = -1;
        for (int k = 0; k < K; ++k) if (!((used >> k) & 1u) && (best < 0 || s2[k] > s2[best])) best = k;
        used |= 1u << best;
        r.nxt[i] = best; o.run_new[i] = s2[best];
    }
    // finished list: best nb of (old finished, stopped continuations of rank < nb)
    int64_t mlen[24];
    for (int i = 0; i < nb; ++i) { msc[i] = r.fsc[i]; mdone[i] = r.fdone[i]; mlen[i] = r.flen[i]; }
    for (int k = 0; k < K; ++k) mlen[nb + k] = cur + 1;
    used = 0;
    for (int i = 0; i < nb; ++i) {
        int best = -1;
        for (int k = 0; k < nb + K; ++k) if (!((used >> k) & 1u) && (best < 0 || msc[k] > msc[best])) best = k;
        used |= 1u << best;
        r.mix[i] = best; o.fsc_new[i] = msc[best]; o.fd_new[i] = mdone[best]; o.fl_new[i] = mlen[best];
    }
    float fmin = o.fsc_new[0];
    bool done_new = true;
    for (int i = 0; i < nb; ++i) { fmin = fminf(fmin, o.fsc_new[i]); done_new = done_new && o.fd_new[i]; }
    // can the best open beam still beat the worst finished one?
    const float best_open = o.run_new[0] / div;
    bool any = false;
    for (int i = 0; i < nb; ++i) any = any || best_open > (o.fd_new[i] ? fmin : NEG);
    o.un = r.unsat && any; o.done_new = done_new; o.all_hits = all_hits;
}

// the log-probability of continuation k's own token: its accumulated score minus its parent beam's OLD running score, one fp32 subtraction
// (kzv/beam.py: top_lp[k] - run_sc[src[k]]; HF compute_transition_scores).  s_old: the nb running scores read before they are replaced.
__device__ __forceinline__ void beam_token_lp(const BeamRank& r, int K, const float* s_old, float* s_tlp) {
    for (int k = 0; k < K; ++k) s_tlp[k] = r.lp[k] - s_old[r.src[k]];
}

// LP: the token rows' log-probability rows go through the same copies (run_lp / fin_lp, double-buffered alike).  The off instance holds
// none of it: no extra LDS, loads or stores.
// PFX (kzv_beam_update_prefix): the image carries a forced prefix, so the generated length is its own: the divisor comes from the table at
// max(cur - prefix_len, 1).  The clamp serves the forced steps, where nothing can finish: they do the running-beam part only and stay
// unsatisfied.  The off instances read neither field.
template <bool LP, bool PFX>
__global__ __launch_bounds__(64) void beam_update_kernel(const BeamUpd p) {
    __shared__ BeamRank r;
    __shared__ float s_old[LP ? 8 : 1], s_tlp[LP ? 16 : 1];
    const int img = blockIdx.x, lane = threadIdx.x;
    const int nb = p.nb, K = p.K, L = p.L;
    if (p.flags[3]) return;                      // the search has ended (beam_stop_kernel): steps issued before the host noticed change nothing
    // the ~40 state words of this image
    beam_rank_load(r, lane, K, nb, img, p.top_lp, p.top_ix, p.fin_sc, p.fin_done, p.fin_len, p.unsat);
    if constexpr (LP) { if (lane >= 40 && lane < 40 + nb) s_old[lane - 40] = p.run_sc[img * nb + lane - 40]; }      // before lane 0 replaces them
    __syncthreads();
    if (lane == 0) {
        BeamRankOut o;
        float div = p.div;
        if constexpr (PFX) div = p.divtab[min(max(p.cur - p.prefix_len[img], 1), L)];
        beam_rank(r, o, nb, K, p.V, p.eos, p.cur, L, p.early, div);
        if constexpr (LP) beam_token_lp(r, K, s_old, s_tlp);
        for (int i = 0; i < nb; ++i) {
            p.rows[img * nb + i] = (int64_t)img * nb + r.src[r.nxt[i]];
            p.run_sc[img * nb + i] = o.run_new[i];
            p.fin_sc[img * nb + i] = o.fsc_new[i]; p.fin_done[img * nb + i] = o.fd_new[i]; p.fin_len[img * nb + i] = o.fl_new[i];
        }
        p.unsat[img] = o.un;
        if (o.un) atomicAdd(p.flags + 0, 1);
        if (!o.done_new) atomicAdd(p.flags + 1, 1);
        if (!o.all_hits) atomicAdd(p.flags + 2, 1);
    }
    __syncthreads();
    // token rows: next running beams = continuation nxt[i]; finished rows = old finished row or a continuation
    for (int i = 0; i < nb; ++i) {
        const int k = r.nxt[i];
        const int64_t* src = p.run_seq_in + ((int64_t)img * nb + r.src[k]) * L;
        int64_t* dst = p.run_seq_out + ((int64_t)img * nb + i) * L;
        for (int j = lane; j < L; j += 64) dst[j] = j == p.cur ? (int64_t)r.tok[k] : src[j];
        const int mi = r.mix[i];
        int64_t* fdst = p.fin_seq_out + ((int64_t)img * nb + i) * L;
        if (mi < nb) {
            const int64_t* fsrc = p.fin_seq_in + ((int64_t)img * nb + mi) * L;
            for (int j = lane; j < L; j += 64) fdst[j] = fsrc[j];
        } else {
            const int kk = mi - nb;
            const int64_t* csrc = p.run_seq_in + ((int64_t)img * nb + r.src[kk]) * L;
            for (int j = lane; j < L; j += 64) fdst[j] = j == p.cur ? (int64_t)r.tok[kk] : csrc[j];
        }
        if constexpr (LP) {                      // the same rows of run_lp / fin_lp, the token's own value at cur
            const float* lsrc = p.run_lp_in + ((int64_t)img * nb + r.src[k]) * L;
            float* ldst = p.run_lp_out + ((int64_t)img * nb + i) * L;
            for (int j = lane; j < L; j += 64) ldst[j] = j == p.cur ? s_tlp[k] : lsrc[j];
            float* lfdst = p.fin_lp_out + ((int64_t)img * nb + i) * L;
            if (mi < nb) {
                const float* lfsrc = p.fin_lp_in + ((int64_t)img * nb + mi) * L;
                for (int j = lane; j < L; j += 64) lfdst[j] = lfsrc[j];
            } else {
                const int kk = mi - nb;
                const float* lcsrc = p.run_lp_in + ((int64_t)img * nb + r.src[kk]) * L;
                for (int j = lane; j < L; j += 64) lfdst[j] = j == p.cur ? s_tlp[kk] : lcsrc[j];
            }
        }
    }
}

// ---- beam search on device-refilled slots (kzv/stream.py::beam_select_seat is the readable statement these are pinned against) ----
// A slot holds an image's whole beam group: decoder rows slot * nb .. slot * nb + nb - 1 at the slot's own step index.  Per step, after
// beam_topk_kernel has ranked every slot's 2 nb continuations: (1) stream_beam_update_kernel, one workgroup per slot: beam_rank at
// cur = slot_t + 1 with the slot's own divisor, then the token rows, the beam row table and the scores in place -- the slot's old rows
// are staged in LDS first, since ONE captured graph serves every step and there is no even / odd buffer to alternate; when the image's
// search has ended, its best finished row and score go to the outputs (NBEST: its n_best best rows, LP: with their per-token
// log-probabilities); (2) stream_beam_seat_kernel, ONE workgroup over all slots:
// stream_seat_kernel's prefix sum, the reset of every reseated slot's beam state, the counters.
struct StreamBeamP {
    const float* top_lp; const int64_t* top_ix;                     // [slots, 2 nb]
    int slots, n_images, nb, L, V, bos, eos, pad, early;
    int* slot_image; int* slot_t; int64_t* tokens; int* posids;     // [slots], [slots * nb]
    int64_t* run_seq; int64_t* fin_seq;                             // [slots, nb, L]
    float* run_sc; float* fin_sc; unsigned char* fin_done; int64_t* fin_len; unsigned char* unsat;
    int* counters;                                                  // next unseated image, searches ended, steps taken, running continuations that took padding
    int* sel;                                                       // [slots][2]: ended, continuations that took padding (update -> seat)
    int64_t* out_ids; int64_t ld_ids; float* out_score; const int* limit;
    const float* div;                                               // [L + 1]: fp32 of n ** length_penalty
    int* rows; int64_t ld_rows;                                     // beam row table [slots * nb, ld_rows] or null
};
// what the NBEST / LP instances of stream_beam_update_kernel take beside it (all null / 0 for the plain instance, which reads none of it)
struct StreamNBestP {
    float* run_lp; float* fin_lp;                                   // [slots, nb, L] fp32: the token rows' log-probability rows (LP)
    int n_best;                                                     // rows 0 .. n_best - 1 of the finished list leave when a search ends
    int64_t* ids; int64_t ld_ids; float* score; int* len;           // [n_images * n_best, ld_ids], [n_images * n_best]
    float* lp; int64_t ld_lp;                                       // optional [n_images * n_best, ld_lp] (LP)
    const int* prefix_len;                                          // [n_images] forced-prefix lengths (PFX), else null
};
constexpr int SB_NB = 4, SB_L = 128;                                // what the staging holds: 2 x 4 x 128 token rows (8 KB) + 4 x 128 table entries; LP: 2 x 4 x 128 fp32 (4 KB) more

// token j of merged finished row mi from the staged rows: an old finished row (mi < nb), or continuation mi - nb = its beam's prefix + the token at cur
__device__ __forceinline__ int64_t beam_fin_token(const BeamRank& r, int mi, int j, int cur, int nb, int L, const int64_t* s_fin, const int64_t* s_run) {
    return mi < nb ? s_fin[mi * L + j] : (j == cur ? (int64_t)r.tok[mi - nb] : s_run[r.src[mi - nb] * L + j]);
}

// its log-probability, from the staged log-probability rows in the same way (s_tlp: the continuations' own values at cur)
__device__ __forceinline__ float beam_fin_lp(const BeamRank& r, int mi, int j, int cur, int nb, int L, const float* s_flp, const float* s_rlp, const float* s_tlp) {
    return mi < nb ? s_flp[mi * L + j] : (j == cur ? s_tlp[mi - nb] : s_rlp[r.src[mi - nb] * L + j]);
}

// NBEST: at the end of a search rows 0 .. n_best - 1 of the finished list leave, not only row 0.  LP (needs NBEST): the log-probability
// rows are staged and moved beside the token rows.  The plain instance <false, false> holds none of either: its LDS and its code are
// those of the kernel without them.
// PFX (kzv_stream_beam_update_prefix): the divisor's index is the image's own generated length max(cur - prefix_len[img], 1), as in
// beam_update_kernel; the off instances do not read the table.
template <bool NBEST, bool LP, bool PFX>
__global__ __launch_bounds__(256) void stream_beam_update_kernel(const StreamBeamP p, const StreamNBestP q) {
    __shared__ BeamRank r;
    __shared__ BeamRankOut o;                    // the ranking lane's results, for every thread
    __shared__ int64_t s_run[SB_NB * SB_L], s_fin[SB_NB * SB_L];
    __shared__ int s_rt[SB_NB * SB_L];
    __shared__ float s_rlp[LP ? SB_NB * SB_L : 1], s_flp[LP ? SB_NB * SB_L : 1], s_old[LP ? 8 : 1], s_tlp[LP ? 16 : 1];
    const int s = blockIdx.x, tid = threadIdx.x;
    const int nb = p.nb, K = 2 * nb, L = p.L;
    const int img = p.slot_image[s];
    if (img < 0) {                               // idle (workgroup-uniform, before any barrier)
        if (tid == 0) { p.sel[2 * s] = 0; p.sel[2 * s + 1] = 0; }
        return;
    }
    const int t = min(p.slot_t[s], L - 2), cur = t + 1;
    const int lim = p.limit ? min(p.limit[img], L) : L;
    const float div = p.div[PFX ? min(max(cur - q.prefix_len[min(img, p.n_images - 1)], 1), L) : cur];
    beam_rank_load(r, tid, K, nb, s, p.top_lp, p.top_ix, p.fin_sc, p.fin_done, p.fin_len, p.unsat);
    // the slot's old rows: whole rows, as the statement moves them (what lies behind cur may be an earlier image's and is never read)
    for (int e = tid; e < nb * L; e += 256) { s_run[e] = p.run_seq[(int64_t)s * nb * L + e]; s_fin[e] = p.fin_seq[(int64_t)s * nb * L + e]; }
    if constexpr (LP) {
        for (int e = tid; e < nb * L; e += 256) { s_rlp[e] = q.run_lp[(int64_t)s * nb * L + e]; s_flp[e] = q.fin_lp[(int64_t)s * nb * L + e]; }
        if (tid >= 40 && tid < 40 + nb) s_old[tid - 40] = p.run_sc[s * nb + tid - 40];      // the old running scores, before they are replaced below
    }
    if (p.rows) for (int e = tid; e < nb * cur; e += 256) { const int i = e / cur, j = e - i * cur; s_rt[i * L + j] = p.rows[((int64_t)s * nb + i) * p.ld_rows + j]; }
    __syncthreads();
    if (tid == 0) {
        BeamRankOut mine; beam_rank(r, mine, nb, K, p.V, p.eos, cur, lim, p.early, div); o = mine;
        if constexpr (LP) beam_token_lp(r, K, s_old, s_tlp);
    }
    __syncthreads();
    const bool go_on = o.un && !(o.done_new && p.early) && !o.all_hits;      // beam_search's go_on, for this image
    if (!go_on) {
        // the best finished hypothesis: only its fl_new[0] tokens (the caller filled BOS / padding; the row behind them may be stale)
        const int mi = r.mix[0], n = (int)o.fl_new[0];
        if (img < p.n_images)
            for (int j = tid; j < min(n, L); j += 256)
                p.out_ids[(int64_t)img * p.ld_ids + j] = beam_fin_token(r, mi, j, cur, nb, L, s_fin, s_run);
        if constexpr (NBEST) {
            // rows 0 .. n_best - 1 of the finished list, each over its own length only; an entry that never received a hypothesis
            // writes no tokens, score -1e9 and length 0 (the host checks for it)
            if (img < p.n_images)
                for (int rr = 0; rr < q.n_best; ++rr) {
                    const int mr = r.mix[rr], nr = o.fd_new[rr] ? min((int)o.fl_new[rr], L) : 0;
                    const int64_t row = (int64_t)img * q.n_best + rr;
                    for (int j = tid; j < nr; j += 256) {
                        q.ids[row * q.ld_ids + j] = beam_fin_token(r, mr, j, cur, nb, L, s_fin, s_run);
                        if constexpr (LP) { if (q.lp) q.lp[row * q.ld_lp + j] = beam_fin_lp(r, mr, j, cur, nb, L, s_flp, s_rlp, s_tlp); }
                    }
                    if (tid == 0) { q.score[row] = o.fd_new[rr] ? o.fsc_new[rr] : -1.0e9f; q.len[row] = nr; }
                }
        }
        if (tid == 0) {
            if (p.out_score && img < p.n_images) p.out_score[img] = o.fsc_new[0];
            p.sel[2 * s] = 1; p.sel[2 * s + 1] = 0;
        }
        return;                                  // the seat kernel puts the slot's beam state back at the start
    }
    for (int e = tid; e < nb * L; e += 256) {
        const int i = e / L, j = e - i * L;
        const int k = r.nxt[i], mi = r.mix[i];
        p.run_seq[(int64_t)s * nb * L + e] = j == cur ? (int64_t)r.tok[k] : s_run[r.src[k] * L + j];
        p.fin_seq[(int64_t)s * nb * L + e] = beam_fin_token(r, mi, j, cur, nb, L, s_fin, s_run);
        if constexpr (LP) {
            q.run_lp[(int64_t)s * nb * L + e] = j == cur ? s_tlp[k] : s_rlp[r.src[k] * L + j];
            q.fin_lp[(int64_t)s * nb * L + e] = beam_fin_lp(r, mi, j, cur, nb, L, s_flp, s_rlp, s_tlp);
        }
    }
    // the row table, kv_rows_kernel's rule with len = slot_t + 1: the step kernel has just written old[b][slot_t] = b; nothing of the cache moves
    if (p.rows) for (int e = tid; e < nb * cur; e += 256) { const int i = e / cur, j = e - i * cur; p.rows[((int64_t)s * nb + i) * p.ld_rows + j] = s_rt[r.src[r.nxt[i]] * L + j]; }
    if (tid < nb) {
        const int i = tid, k = r.nxt[i];
        p.run_sc[s * nb + i] = o.run_new[i]; p.fin_sc[s * nb + i] = o.fsc_new[i]; p.fin_done[s * nb + i] = o.fd_new[i]; p.fin_len[s * nb + i] = o.fl_new[i];
        p.tokens[s * nb + i] = r.tok[k]; p.posids[s * nb + i] = cur + 1 + p.pad;
    }
    if (tid == 0) {
        int npad = 0;                            // a running prefix with padding breaks "position = step + 1 + pad, every cached key usable"
        for (int i = 0; i < nb; ++i) npad += (r.tok[r.nxt[i]] == p.pad && !r.hit[r.nxt[i]]) ? 1 : 0;
        p.unsat[s] = o.un;
        p.sel[2 * s] = 0; p.sel[2 * s + 1] = npad;
    }
}

// a slot's beam state at the start of a search (new_beam_state); the token rows keep what they hold: column 0 is BOS from the first seating on
__device__ __forceinline__ void stream_beam_reset(const StreamBeamP& p, int s) {
    for (int i = 0; i < p.nb; ++i) {
        p.run_sc[s * p.nb + i] = i == 0 ? 0.f : -1.0e9f; p.fin_sc[s * p.nb + i] = -1.0e9f; p.fin_done[s * p.nb + i] = 0; p.fin_len[s * p.nb + i] = 1;
        p.tokens[s * p.nb + i] = p.bos; p.posids[s * p.nb + i] = p.pad + 1;
    }
    p.unsat[s] = 1; p.slot_t[s] = 0;
}

__global__ __launch_bounds__(256) void stream_beam_seat_kernel(const StreamBeamP p) {
    __shared__ int s_w[4], s_pad;
    const int tid = threadIdx.x, next = p.counters[0];
    if (tid == 0) s_pad = 0;
    int carry = 0;                               // searches ended in the slots below this pass
    for (int base = 0; base < p.slots; base += 256) {
        const int s = base + tid;
        const bool in = s < p.slots;
        const int e = in ? p.sel[2 * s] : 0;
        int total;
        const int rank = carry + seat_rank(e != 0, tid, s_w, total);      // ended slots below slot s
        if (in) {
            if (e) {
                const int ni = next + rank;
                p.slot_image[s] = ni < p.n_images ? ni : -1;
                stream_beam_reset(p, s);
            } else if (p.slot_image[s] >= 0) {
                p.slot_t[s] += 1;
                if (p.sel[2 * s + 1]) atomicAdd(&s_pad, p.sel[2 * s + 1]);
            }
        }
        carry += total;
        __syncthreads();
    }
    if (tid == 0) {
        seat_counters(p.counters, next, carry, p.n_images);
        p.counters[3] += s_pad;
    }
}

// the first min(slots, n_images) images take the slots in order, every slot's beam state at the start, the token rows BOS + padding
__global__ void stream_beam_start_kernel(const StreamBeamP p, const StreamNBestP q) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e < p.slots * p.nb * p.L) { const int64_t v = e % p.L == 0 ? p.bos : p.pad; p.run_seq[e] = v; p.fin_seq[e] = v; }
    if (q.run_lp && e < p.slots * p.nb * p.L) { q.run_lp[e] = 0.f; q.fin_lp[e] = 0.f; }      // column 0 is never written again: it stays 0
    if (e < p.slots) { p.slot_image[e] = e < p.n_images ? e : -1; stream_beam_reset(p, e); }
    if (e == 0) { p.counters[0] = min(p.slots, p.n_images); p.counters[1] = 0; p.counters[2] = 0; p.counters[3] = 0; }
}

// inputs of decoder step t from the token table: newest token, its RoBERTa position id (HF modeling_roberta.py:142-155: t + 1 +
// pad_id for a real token, pad_id for padding) and the key-usable flag of column t -- six small torch kernels otherwise
__global__ void decode_prep_kernel(const int64_t* __restrict__ ids, int64_t ld_ids, int t, int pad, int B, int64_t* __restrict__ tok,
                                   unsigned char* __restrict__ valid, int64_t ld_valid, int* __restrict__ posids) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    const int64_t v = ids[(int64_t)b * ld_ids + t];
    const bool live = v != pad;
    tok[b] = v;
    valid[(int64_t)b * ld_valid + t] = live ? 1 : 0;
    posids[b] = live ? t + 1 + pad : pad;
}

// greedy token selection of one sequence (the num_beams = 1 branch of HF _sample: argmax, padding once the sequence has ended):
// the first index of the row maximum, like torch.argmax
__global__ __launch_bounds__(256) void greedy_update_kernel(const float* __restrict__ logits, int64_t ld, int V, int64_t* __restrict__ ids, int64_t ld_ids,
                                                            int t, unsigned char* __restrict__ done, int pad, int eos, int* __restrict__ flags) {
    __shared__ float s_v[4]; __shared__ int s_i[4];
    const int b = blockIdx.x, tid = threadIdx.x;
    float bv; int bi;
    row_first_argmax<8>(logits + (int64_t)b * ld, V, tid, s_v, s_i, bv, bi);
    if (tid == 0) {
        const bool was = done[b] != 0;
        const int nxt = was ? pad : bi;
        ids[(int64_t)b * ld_ids + t + 1] = nxt;
        const bool now = was || nxt == eos;
        done[b] = now ? 1 : 0;
        if (!now) atomicAdd(flags + t, 1);
    }
}

// after beam_update: the loop condition of HF _beam_search, kept on the device so that the host may look only every few steps
__global__ void beam_stop_kernel(int* flags, int early, int cur) {
    if (flags[3]) return;
    flags[4] = cur;                              // updates applied so far (cur counts from 1)
    const bool go_on = flags[0] > 0 && !(early && flags[1] == 0) && flags[2] > 0;
    if (!go_on) flags[3] = 1;
}

}  // namespace

// what both slot states owe: their device arrays and out_ids, positive sizes, max_len columns (2 .. cap, 0: no cap) within the shortest output row
static int slot_state_check(const char* who, int slots, int n_images, int vocab, int max_len, int cap, int64_t ld_out, const void* out_ids,
                            std::initializer_list<const void*> arrays) {
    for (const void* a : arrays) if (!a) return kzv_fail(KZV_E_ARG, "%s: null state array", who);
    if (!out_ids) return kzv_fail(KZV_E_ARG, "%s: null out_ids", who);
    if (slots < 1 || n_images < 1 || vocab < 1) return kzv_fail(KZV_E_ARG, "%s: slots, images and vocabulary must be positive", who);
    if (max_len < 2 || (cap && max_len > cap) || ld_out < max_len)
        return cap ? kzv_fail(KZV_E_ARG, "%s: max_len 2..%d columns within the output rows", who, cap) : kzv_fail(KZV_E_ARG, "%s: max_len >= 2 columns within the output rows", who);
    return KZV_OK;
}

static int stream_params(const kzv_stream_state* st, const float* d_logits, int64_t ld, StreamP* p, const char* who) {
    if (!st) return kzv_fail(KZV_E_ARG, "%s: null state", who);
    KZV_TRY_RC(slot_state_check(who, st->slots, st->n_images, st->vocab, st->max_len, 0, st->out_logprob && st->ld_logprob < st->ld_ids ? st->ld_logprob : st->ld_ids,
                                st->out_ids, {st->slot_image, st->slot_t, st->tokens, st->posids, st->counters, st->scratch}));
    *p = StreamP{d_logits, ld, st->vocab, st->slots, st->n_images, st->max_len, st->bos_id, st->eos_id, st->pad_id, st->slot_image, st->slot_t, st->tokens,
                 st->posids, st->counters, st->scratch, st->out_ids, st->ld_ids, st->out_logprob, st->ld_logprob, st->limit};
    return KZV_OK;
}

extern "C" int kzv_stream_seat_first(const kzv_stream_state* st, void* stream) {
    StreamP p;
    KZV_TRY_RC(stream_params(st, nullptr, 0, &p, "stream_seat_first"));
    hipLaunchKernelGGL(stream_start_kernel, dim3((st->slots + 255) / 256), dim3(256), 0, (hipStream_t)stream, p);
    return kzv_check_launch("stream_seat_first");
}

extern "C" int kzv_stream_update(const kzv_stream_state* st, const float* d_logits, int64_t ld, void* stream) {
    StreamP p;
    KZV_TRY_RC(stream_params(st, d_logits, ld, &p, "stream_update"));
    if (!d_logits || ld < st->vocab) return kzv_fail(KZV_E_ARG, "stream_update: logits [slots, ld >= vocab]");
    hipLaunchKernelGGL(stream_select_kernel, dim3(st->slots), dim3(256), 0, (hipStream_t)stream, p);
    hipLaunchKernelGGL(stream_seat_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, p);
    return kzv_check_launch("stream_update");
}

static int stream_beam_params(const kzv_stream_beam_state* st, const float* top_lp, const int64_t* top_ix, StreamBeamP* p, StreamNBestP* q, const char* who) {
    if (!st) return kzv_fail(KZV_E_ARG, "%s: null state", who);
    KZV_TRY_RC(slot_state_check(who, st->slots, st->n_images, st->vocab, st->max_len, SB_L, st->ld_ids, st->out_ids,
                                {st->slot_image, st->slot_t, st->tokens, st->posids, st->run_seq, st->fin_seq, st->run_scores, st->fin_scores, st->fin_done,
                                 st->fin_len, st->unsatisfied, st->counters, st->scratch}));
    if (!st->divisors) return kzv_fail(KZV_E_ARG, "%s: null divisors (fp32 [max_len + 1] of n ** length_penalty)", who);
    if (st->num_beams != 2 && st->num_beams != 4) return kzv_fail(KZV_E_ARG, "%s: num_beams %d: a slot holds 2 or 4 beams", who, st->num_beams);
    if ((int64_t)st->slots * st->num_beams * st->max_len >= (1ll << 31) || (int64_t)st->num_beams * st->vocab >= (1ll << 31)) return kzv_fail(KZV_E_ARG, "%s: state beyond 32-bit indices", who);
    if (st->rows && st->ld_rows < st->max_len - 1) return kzv_fail(KZV_E_ARG, "%s: row table rows shorter than the max_len - 1 steps", who);
    *p = StreamBeamP{top_lp, top_ix, st->slots, st->n_images, st->num_beams, st->max_len, st->vocab, st->bos_id, st->eos_id, st->pad_id, st->early_stopping ? 1 : 0,
                     st->slot_image, st->slot_t, st->tokens, st->posids, st->run_seq, st->fin_seq, st->run_scores, st->fin_scores, st->fin_done, st->fin_len,
                     st->unsatisfied, st->counters, st->scratch, st->out_ids, st->ld_ids, st->out_score, st->limit, st->divisors, st->rows, st->ld_rows};
    // the n-best outputs and the log-probability rows: n_best == 0 and every pointer null is the state without them
    const bool lp_rows = st->run_lp || st->fin_lp;
    if (st->n_best == 0) {
        if (lp_rows || st->nbest_ids || st->nbest_scores || st->nbest_len || st->nbest_logprob)
            return kzv_fail(KZV_E_ARG, "%s: n-best arrays or log-probability rows with n_best == 0", who);
    } else {
        if (st->n_best < 1 || st->n_best > st->num_beams) return kzv_fail(KZV_E_ARG, "%s: n_best %d outside 1..num_beams = %d", who, st->n_best, st->num_beams);
        if (!st->nbest_ids || !st->nbest_scores || !st->nbest_len) return kzv_fail(KZV_E_ARG, "%s: null n-best ids / scores / lengths", who);
        if (st->ld_nbest < st->max_len) return kzv_fail(KZV_E_ARG, "%s: n-best rows shorter than max_len", who);
        if (lp_rows && (!st->run_lp || !st->fin_lp)) return kzv_fail(KZV_E_ARG, "%s: run_lp and fin_lp come together", who);
        if (st->nbest_logprob && !lp_rows) return kzv_fail(KZV_E_ARG, "%s: nbest_logprob needs the log-probability rows run_lp / fin_lp", who);
        if (st->nbest_logprob && st->ld_nbest_logprob < st->max_len) return kzv_fail(KZV_E_ARG, "%s: n-best log-probability rows shorter than max_len", who);
        if ((int64_t)st->n_images * st->n_best >= (1ll << 31)) return kzv_fail(KZV_E_ARG, "%s: n-best rows beyond 32-bit indices", who);
    }
    *q = StreamNBestP{st->run_lp, st->fin_lp, st->n_best, st->nbest_ids, st->ld_nbest, st->nbest_scores, st->nbest_len, st->nbest_logprob, st->ld_nbest_logprob, nullptr};
    return KZV_OK;
}

extern "C" int kzv_stream_beam_seat_first(const kzv_stream_beam_state* st, void* stream) {
    StreamBeamP p; StreamNBestP q;
    KZV_TRY_RC(stream_beam_params(st, nullptr, nullptr, &p, &q, "stream_beam_seat_first"));
    hipLaunchKernelGGL(stream_beam_start_kernel, dim3((st->slots * st->num_beams * st->max_len + 255) / 256), dim3(256), 0, (hipStream_t)stream, p, q);
    return kzv_check_launch("stream_beam_seat_first");
}

template <bool PFX>
static int stream_beam_update_launch(const char* who, const kzv_stream_beam_state* st, const float* d_top_scores, const int64_t* d_top_index,
                                     const int32_t* d_prefix_len, void* stream) {
    StreamBeamP p; StreamNBestP q;
    KZV_TRY_RC(stream_beam_params(st, d_top_scores, d_top_index, &p, &q, who));
    if (!d_top_scores || !d_top_index) return kzv_fail(KZV_E_ARG, "%s: null ranking [slots, 2 * num_beams]", who);
    q.prefix_len = PFX ? d_prefix_len : nullptr;
    if (q.run_lp) hipLaunchKernelGGL((stream_beam_update_kernel<true, true, PFX>), dim3(st->slots), dim3(256), 0, (hipStream_t)stream, p, q);
    else if (q.n_best) hipLaunchKernelGGL((stream_beam_update_kernel<true, false, PFX>), dim3(st->slots), dim3(256), 0, (hipStream_t)stream, p, q);
    else hipLaunchKernelGGL((stream_beam_update_kernel<false, false, PFX>), dim3(st->slots), dim3(256), 0, (hipStream_t)stream, p, q);
    hipLaunchKernelGGL(stream_beam_seat_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, p);
    return kzv_check_launch(who);
}

extern "C" int kzv_stream_beam_update(const kzv_stream_beam_state* st, const float* d_top_scores, const int64_t* d_top_index, void* stream) {
    return stream_beam_update_launch<false>("stream_beam_update", st, d_top_scores, d_top_index, nullptr, stream);
}

extern "C" int kzv_stream_beam_update_prefix(const kzv_stream_beam_state* st, const float* d_top_scores, const int64_t* d_top_index,
                                             const int32_t* d_prefix_len, void* stream) {
    if (!d_prefix_len) return stream_beam_update_launch<false>("stream_beam_update_prefix", st, d_top_scores, d_top_index, nullptr, stream);
    return stream_beam_update_launch<true>("stream_beam_update_prefix", st, d_top_scores, d_top_index, d_prefix_len, stream);
}

static int beam_topk_args(const char* who, const float* d_logits, int64_t ld, const float* d_beam_scores, int batch, int num_beams, int vocab, int k,
                          const float* d_top_scores, const int64_t* d_top_index) {
    if (!d_logits || !d_beam_scores || !d_top_scores || !d_top_index) return kzv_fail(KZV_E_ARG, "%s: null operand", who);
    if (batch < 1 || num_beams < 1 || num_beams > 8 || vocab < 1 || ld < vocab) return kzv_fail(KZV_E_ARG, "%s: 1..8 beams, ld >= vocab", who);
    if (k < 1 || k > 16 || (int64_t)k > (int64_t)num_beams * vocab) return kzv_fail(KZV_E_ARG, "%s: 1..16 continuations, at most beams * vocab", who);
    if ((int64_t)num_beams * vocab >= (1ll << 31)) return kzv_fail(KZV_E_ARG, "%s: beams * vocab beyond 32-bit flat indices", who);
    if (vocab > 64 * 256) return kzv_fail(KZV_E_ARG, "%s: vocab beyond 16,384", who);
    return KZV_OK;
}

template <bool LSE>
static int beam_topk_launch(const char* who, const float* d_logits, int64_t ld, const float* d_beam_scores, int batch, int num_beams, int vocab, int k,
                            float* d_top_scores, int64_t* d_top_index, void* stream) {
    const int rc = beam_topk_args(who, d_logits, ld, d_beam_scores, batch, num_beams, vocab, k, d_top_scores, d_top_index);
    if (rc != KZV_OK) return rc;
    hipStream_t s = (hipStream_t)stream;
#define KZV_BT(KM, E) hipLaunchKernelGGL((beam_topk_kernel<KM, E, LSE>), dim3(batch), dim3(256), 0, s, d_logits, ld, d_beam_scores, num_beams, vocab, k, d_top_scores, d_top_index)
#define KZV_BT_E(KM) do { if (vocab <= 4 * 256) KZV_BT(KM, 4); else if (vocab <= 20 * 256) KZV_BT(KM, 20); else KZV_BT(KM, 64); } while (0)
    if (k <= 4) KZV_BT_E(4);
    else if (k <= 8) KZV_BT_E(8);
    else KZV_BT_E(16);
#undef KZV_BT_E
#undef KZV_BT
    return kzv_check_launch(who);
}

extern "C" int kzv_beam_topk(const float* d_logits, int64_t ld, const float* d_beam_scores, int batch, int num_beams, int vocab, int k,
                             float* d_top_scores, int64_t* d_top_index, void* stream) {
    return beam_topk_launch<true>("beam_topk", d_logits, ld, d_beam_scores, batch, num_beams, vocab, k, d_top_scores, d_top_index, stream);
}

extern "C" int kzv_beam_rank_logprobs(const float* d_logprobs, int64_t ld, const float* d_beam_scores, int batch, int num_beams, int vocab, int k,
                                      float* d_top_scores, int64_t* d_top_index, void* stream) {
    return beam_topk_launch<false>("beam_rank_logprobs", d_logprobs, ld, d_beam_scores, batch, num_beams, vocab, k, d_top_scores, d_top_index, stream);
}

static int beam_update_launch(const char* who, const kzv_beam_state* st, const float* d_top_scores, const int64_t* d_top_index, int cur, int early_stopping,
                              float length_penalty, const float* d_divisors, const int32_t* d_prefix_len, int64_t* d_rows, int* d_flags, void* stream) {
    if (!st || !d_top_scores || !d_top_index || !d_rows || !d_flags) return kzv_fail(KZV_E_ARG, "%s: null operand", who);
    if (!st->run_seq_in || !st->run_seq_out || !st->fin_seq_in || !st->fin_seq_out || !st->run_scores || !st->fin_scores || !st->fin_done ||
        !st->fin_len || !st->unsatisfied) return kzv_fail(KZV_E_ARG, "%s: null state array", who);
    if (st->batch < 1 || st->num_beams < 1 || st->num_beams > 8 || st->max_len < 2 || st->vocab < 1) return kzv_fail(KZV_E_ARG, "%s: 1..8 beams", who);
    if (cur < 1 || cur >= st->max_len) return kzv_fail(KZV_E_ARG, "%s: position outside 1..max_len-1", who);
    if (st->run_seq_in == st->run_seq_out || st->fin_seq_in == st->fin_seq_out) return kzv_fail(KZV_E_ARG, "%s: in and out token rows must differ", who);
    const bool lp_rows = st->run_lp_in || st->run_lp_out || st->fin_lp_in || st->fin_lp_out;
    if (lp_rows && (!st->run_lp_in || !st->run_lp_out || !st->fin_lp_in || !st->fin_lp_out)) return kzv_fail(KZV_E_ARG, "%s: the four log-probability row arrays come together", who);
    if (lp_rows && (st->run_lp_in == st->run_lp_out || st->fin_lp_in == st->fin_lp_out)) return kzv_fail(KZV_E_ARG, "%s: in and out log-probability rows must differ", who);
    hipStream_t s = (hipStream_t)stream;
    if (hipMemsetAsync(d_flags, 0, (cur == 1 ? 5 : 3) * sizeof(int), s) != hipSuccess) return kzv_fail(KZV_E_HIP, "%s: memset", who);
    BeamUpd p{d_top_scores, d_top_index, st->run_seq_in, st->run_seq_out, st->fin_seq_in, st->fin_seq_out, st->run_scores, st->fin_scores,
              st->fin_done, st->fin_len, st->unsatisfied, d_rows, d_flags, st->num_beams, 2 * st->num_beams, st->max_len, st->vocab, cur,
              st->eos_id, early_stopping ? 1 : 0, (float)pow((double)cur, (double)length_penalty),
              st->run_lp_in, st->run_lp_out, st->fin_lp_in, st->fin_lp_out, d_prefix_len, d_divisors};
    if (d_prefix_len) {
        if (lp_rows) hipLaunchKernelGGL((beam_update_kernel<true, true>), dim3(st->batch), dim3(64), 0, s, p);
        else hipLaunchKernelGGL((beam_update_kernel<false, true>), dim3(st->batch), dim3(64), 0, s, p);
    } else {
        if (lp_rows) hipLaunchKernelGGL((beam_update_kernel<true, false>), dim3(st->batch), dim3(64), 0, s, p);
        else hipLaunchKernelGGL((beam_update_kernel<false, false>), dim3(st->batch), dim3(64), 0, s, p);
    }
    hipLaunchKernelGGL(beam_stop_kernel, dim3(1), dim3(1), 0, s, d_flags, early_stopping ? 1 : 0, cur);
    return kzv_check_launch(who);
}

extern "C" int kzv_beam_update(const kzv_beam_state* st, const float* d_top_scores, const int64_t* d_top_index, int cur, int early_stopping,
                               float length_penalty, int64_t* d_rows, int* d_flags, void* stream) {
    return beam_update_launch("beam_update", st, d_top_scores, d_top_index, cur, early_stopping, length_penalty, nullptr, nullptr, d_rows, d_flags, stream);
}

extern "C" int kzv_beam_update_prefix(const kzv_beam_state* st, const float* d_top_scores, const int64_t* d_top_index, int cur, int early_stopping,
                                      float length_penalty, const float* d_divisors, const int32_t* d_prefix_len, int64_t* d_rows, int* d_flags, void* stream) {
    if (d_prefix_len && !d_divisors) return kzv_fail(KZV_E_ARG, "beam_update_prefix: prefix lengths need the divisor table (fp32 [max_len + 1] of n ** length_penalty)");
    return beam_update_launch("beam_update_prefix", st, d_top_scores, d_top_index, cur, early_stopping, length_penalty, d_divisors, d_prefix_len, d_rows, d_flags, stream);
}

extern "C" int kzv_decode_prep(const int64_t* d_ids, int64_t ld_ids, int t, int pad_id, int batch, int64_t* d_tokens, uint8_t* d_valid, int64_t ld_valid,
                               int32_t* d_posids, void* stream) {
    if (!d_ids || !d_tokens || !d_valid || !d_posids || batch < 1 || t < 0 || t >= ld_ids || t >= ld_valid) return kzv_fail(KZV_E_ARG, "decode_prep: bad arguments");
    hipLaunchKernelGGL(decode_prep_kernel, dim3((batch + 255) / 256), dim3(256), 0, (hipStream_t)stream, d_ids, ld_ids, t, pad_id, batch, d_tokens, d_valid, ld_valid, d_posids);
    return kzv_check_launch("decode_prep");
}

extern "C" int kzv_greedy_update(const float* d_logits, int64_t ld, int vocab, int64_t* d_ids, int64_t ld_ids, int t, uint8_t* d_done, int batch,
                                 int pad_id, int eos_id, int32_t* d_flags, void* stream) {
    if (!d_logits || !d_ids || !d_done || !d_flags || batch < 1 || vocab < 1 || ld < vocab || t < 0 || t + 1 >= ld_ids) return kzv_fail(KZV_E_ARG, "greedy_update: bad arguments");
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(greedy_update_kernel, dim3(batch), dim3(256), 0, s, d_logits, ld, vocab, d_ids, ld_ids, t, d_done, pad_id, eos_id, d_flags);
    return kzv_check_launch("greedy_update");
}
