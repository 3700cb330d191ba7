// Slot-refill decoding on the model handle (include/kzv.h: kzv_stream_*): greedy, one row per slot; or beam search, a slot holding an
// image's beam group.  A wave's begin, its options (StreamWaveOpts), the score chain between the vocabulary GEMM and the selection, the
// step and its graph replay, the poll.  The cache, the weight packs and the capture helper are model_decode.cpp's (model_internal.h).
#include "model_internal.h"
#include <type_traits>

static bool stream_supported(const kzv_model* m, int nb = 1) {
    return decode_one_launch_mode() && kzv_decode_fused_supported(m->Hd, m->c.dec_heads, m->Fd, m->Ld, nb, m->T, m->npa) &&
           (nb == 1 || ((nb == 2 || nb == 4) && m->B % nb == 0 && m->V <= 64 * 256));       // kzv_beam_topk ranks up to 16,384 columns
}
extern "C" int kzv_stream_decode_impl(const kzv_model* m) {
    if (!m || !m->bound) return kzv_fail(KZV_E_STATE, "stream_decode_impl: model not bound");
    return stream_supported(m) ? 1 : 0;
}
extern "C" int kzv_stream_beam_impl(const kzv_model* m, int num_beams) {
    if (!m || !m->bound) return kzv_fail(KZV_E_STATE, "stream_beam_impl: model not bound");
    return (num_beams == 2 || num_beams == 4) && stream_supported(m, num_beams) ? 1 : 0;
}
static bool stream_e4m3(const kzv_model* m) { return m->dec_weights == KZV_DECODE_WEIGHTS_E4M3; }

// every entry that needs a wave in progress: `hint` names the call that begins one
static int wave_check(const kzv_model* m, const char* who, const char* hint) {
    return m && m->bound && m->swave ? KZV_OK : kzv_fail(KZV_E_STATE, "%s: call %s first", who, hint);
}

// What the wave's rows are, whichever kind it is: a greedy wave's histories are the rows of out_ids, one per IMAGE; a beam wave's are
// the rows of run_seq, one per row.  The one place that tells sst from sbst after kzv_stream_begin.
struct WaveRows {
    const int64_t* ids; int64_t ld_ids;
    int group, by_image, n_images, eos_id, max_len;
    const int32_t* slot_image; const int32_t* slot_t;
    int64_t* tokens; int32_t* posids; int32_t* counters;
    explicit WaveRows(const kzv_model* m) {
        const auto common = [this](const auto& st) {
            n_images = st.n_images; eos_id = st.eos_id; max_len = st.max_len; slot_image = st.slot_image; slot_t = st.slot_t;
            tokens = st.tokens; posids = st.posids; counters = st.counters;
        };
        if (!m->sbeams) { common(m->sst); ids = m->sst.out_ids; ld_ids = m->sst.ld_ids; group = 1; by_image = 1; }
        else { common(m->sbst); ids = m->sbst.run_seq; ld_ids = m->sbst.max_len; group = m->sbeams; by_image = 0; }
    }
};

// the fields the three score nodes' arguments have in common: the step's logits and where each row's slot lies
template <typename Args>
static void fill_rows(Args& a, const kzv_model* m, const WaveRows& w) {
    memset(&a, 0, sizeof(a));
    a.logits = m->slogits; a.ld = m->V; a.rows = m->B; a.vocab = m->V;
    a.group = w.group; a.slot_image = w.slot_image; a.slot_t = w.slot_t; a.by_image = w.by_image; a.n_images = w.n_images;
}

// The slot state inside kzv_model::sstate, carved in order from `base`: logits [B, V] (256-byte block), then the 8-byte words, then the
// 4-byte ones, then bytes.  Run on a null base it only counts (the bytes the layout needs for rows of `len` tokens), run on the reserved
// block it places the pointers of m->sst / m->sbst: size and layout come from the same lines.  *div: a beam wave's divisor table.
static size_t carve_slots(kzv_model* m, char* base, int nb, int len, float** div) {
    size_t off = 0;
    const auto take = [&](auto*& p, size_t n, size_t pad = 1) {
        p = base ? (std::remove_reference_t<decltype(p)>)(base + off) : nullptr;
        off += align_up(n * sizeof(*p), pad);
    };
    const size_t B = m->B, slots = B / nb;
    take(m->slogits, B * m->V, 256);
    if (nb == 1) {
        kzv_stream_state& st = m->sst;
        take(st.tokens, B);
        take(st.slot_image, B); take(st.slot_t, B); take(st.posids, B); take(st.scratch, 2 * B); take(st.counters, 4);
    } else {
        kzv_stream_beam_state& st = m->sbst;
        take(st.tokens, B); take(st.run_seq, B * len); take(st.fin_seq, B * len); take(st.fin_len, B); take(m->stop_ix, 2 * B);
        take(st.run_scores, B); take(st.fin_scores, B); take(m->stop_lp, 2 * B);
        take(st.posids, B); take(st.slot_image, slots); take(st.slot_t, slots); take(st.scratch, 2 * slots); take(st.counters, 4);
        take(*div, (size_t)len + 1, 8);
        take(st.fin_done, B); take(st.unsatisfied, B);
    }
    return off;
}

// nb = 1: kzv_stream_begin; nb = 2 / 4: kzv_stream_begin_beams (slots = bound batch / nb)
static int stream_begin(kzv_model* m, const char* who, int nb, int early, float length_penalty, float* d_out_scores, int pool_images, int n_images, int max_len,
                        int bos_id, int eos_id, int64_t* d_out_ids, int64_t ld_ids, float* d_out_logprob, int64_t ld_logprob, const int32_t* d_limit,
                        void* stream) {
    // what needs no bound state first: these are argument errors on any handle
    if (!m) return kzv_fail(KZV_E_ARG, "%s: null model", who);
    if (nb != 1 && nb != 2 && nb != 4) return kzv_fail(KZV_E_ARG, "%s: num_beams %d: a slot holds 2 or 4 beams", who, nb);
    if (!d_out_ids) return kzv_fail(KZV_E_ARG, "%s: null out_ids", who);
    if (max_len < 2) return kzv_fail(KZV_E_ARG, "%s: max_len %d: a line is BOS and at least one token", who, max_len);
    if (n_images < 1 || n_images > pool_images) return kzv_fail(KZV_E_ARG, "%s: a wave of %d images for a pool of %d", who, n_images, pool_images);
    if (ld_ids < max_len || (d_out_logprob && ld_logprob < max_len)) return kzv_fail(KZV_E_ARG, "%s: output rows shorter than max_len", who);
    if (nb > 1 && d_out_logprob) return kzv_fail(KZV_E_ARG, "%s: a beam search returns no per-token log-probabilities (d_out_logprob must be null)", who);
    if (!m->bound) return kzv_fail(KZV_E_STATE, "%s: model not bound", who);
    m->swave = false;
    if (m->B % nb) return kzv_fail(KZV_E_ARG, "%s: the %d bound rows are no multiple of %d beams", who, m->B, nb);
    const int B = m->B, V = m->V, slots = B / nb;
    if (pool_images < slots) return kzv_fail(KZV_E_ARG, "%s: a pool of %d images is smaller than the %d slots", who, pool_images, slots);
    if (bos_id < 0 || bos_id >= m->V || eos_id < 0 || eos_id >= m->V) return kzv_fail(KZV_E_ARG, "%s: BOS / EOS outside the vocabulary", who);
    if (max_len > m->L) return kzv_fail(KZV_E_ARG, "%s: max_len %d outside 2..%d (the bound length)", who, max_len, m->L);
    if (max_len - 1 + m->c.pad_id >= m->c.max_pos) return kzv_fail(KZV_E_ARG, "%s: max_len %d needs position id %d, the table has %d rows", who, max_len, max_len - 1 + m->c.pad_id, m->c.max_pos);
    if (!stream_supported(m, nb)) return kzv_fail(KZV_E_STATE, "%s: this geometry has no slot-refill decoding (kzv_stream_decode_impl / kzv_stream_beam_impl)", who);
    hipStream_t s = (hipStream_t)stream;
    drop_stream_graph(m);                        // it holds the last wave's outputs and counts
    const size_t bytes = (size_t)m->Ld * 2 * pool_images * m->npa * m->Hd * sizeof(bf16_t);
    if (!reserve(m, m->spool, bytes)) return kzv_fail(KZV_E_HIP, "%s: pool allocation (%zu bytes)", who, bytes);
    m->spool_images = pool_images;
    // sized for rows of the bound length (max_len <= L, checked above), so that a longer wave on the same handle moves nothing
    float* div = nullptr;
    const size_t sb = carve_slots(m, nullptr, nb, m->L, &div);
    if (!m->sstate || m->sstate_slots < B || m->sstate_V < V || m->sstate.capacity() < sb) {
        if (!reserve(m, m->sstate, sb)) return kzv_fail(KZV_E_HIP, "%s: slot state allocation (%zu bytes)", who, sb);
        m->sstate_slots = B; m->sstate_V = V;
    }
    carve_slots(m, m->sstate.as<char>(), nb, max_len, &div);
    m->sbeams = nb > 1 ? nb : 0;
    m->sopt = StreamWaveOpts{};                  // every kzv_stream_set_* belongs to one wave ...
    m->sbst.n_best = 0; m->sbst.run_lp = m->sbst.fin_lp = nullptr;      // ... and so does kzv_stream_set_nbest, whose fields are the public state's
    m->sbst.nbest_ids = nullptr; m->sbst.ld_nbest = 0; m->sbst.nbest_scores = nullptr; m->sbst.nbest_len = nullptr; m->sbst.nbest_logprob = nullptr; m->sbst.ld_nbest_logprob = 0;
    if (nb == 1) {
        kzv_stream_state& st = m->sst;
        st.slots = B; st.n_images = n_images; st.max_len = max_len; st.vocab = V; st.pad_id = m->c.pad_id; st.bos_id = bos_id; st.eos_id = eos_id; st.reserved = 0;
        st.out_ids = d_out_ids; st.ld_ids = ld_ids; st.out_logprob = d_out_logprob; st.ld_logprob = ld_logprob; st.limit = d_limit;
    } else {
        kzv_stream_beam_state& st = m->sbst;
        st.slots = slots; st.n_images = n_images; st.num_beams = nb; st.max_len = max_len; st.vocab = V; st.pad_id = m->c.pad_id; st.bos_id = bos_id;
        st.eos_id = eos_id; st.early_stopping = early ? 1 : 0;
        st.out_ids = d_out_ids; st.ld_ids = ld_ids; st.out_score = d_out_scores; st.limit = d_limit; st.divisors = div;
        // the divisors kzv_beam_update takes per call: (float)pow((double)n, (double)length_penalty), as a table since every slot has its own n
        m->sdiv.assign((size_t)max_len + 1, 1.f);
        for (int n = 1; n <= max_len; ++n) m->sdiv[n] = (float)pow((double)n, (double)length_penalty);
        if (hipMemcpyAsync(div, m->sdiv.data(), sizeof(float) * m->sdiv.size(), hipMemcpyHostToDevice, s) != hipSuccess) return kzv_fail(KZV_E_HIP, "%s: divisor table copy", who);
    }
    KZV_TRY(ensure_kv_cache(m));
    if (nb > 1) { m->sbst.rows = m->rowtab[0].as<int>(); m->sbst.ld_rows = m->T; }       // ensure_kv_cache may have moved it
    KZV_TRY(ensure_dec_pack(m, s));
    if (stream_e4m3(m)) KZV_TRY(build_dec_pack8(m, s));
    m->rt_cur = -1;
    if (hipMemsetAsync(m->hd_gelu, 0, sizeof(float) * (size_t)B * m->Hd, s) != hipSuccess) return kzv_fail(KZV_E_HIP, "%s: memset", who);
    m->train = false; m->have_fwd = false; m->have_dec = false;
    m->swave = true;
    return KZV_OK;
}

extern "C" int kzv_stream_begin(kzv_model* m, int pool_images, int n_images, int max_len, int bos_id, int eos_id, int64_t* d_out_ids, int64_t ld_ids,
                                float* d_out_logprob, int64_t ld_logprob, const int32_t* d_limit, void* stream) {
    return stream_begin(m, "stream_begin", 1, 0, 1.f, nullptr, pool_images, n_images, max_len, bos_id, eos_id, d_out_ids, ld_ids, d_out_logprob, ld_logprob,
                        d_limit, stream);
}

extern "C" int kzv_stream_begin_beams(kzv_model* m, int num_beams, int early_stopping, float length_penalty, float* d_out_scores, int pool_images,
                                      int n_images, int max_len, int bos_id, int eos_id, int64_t* d_out_ids, int64_t ld_ids, float* d_out_logprob,
                                      int64_t ld_logprob, const int32_t* d_limit, void* stream) {
    if (num_beams != 2 && num_beams != 4) return kzv_fail(KZV_E_ARG, "stream_begin_beams: num_beams %d: a slot holds 2 or 4 beams", num_beams);
    return stream_begin(m, "stream_begin_beams", num_beams, early_stopping, length_penalty, d_out_scores, pool_images, n_images, max_len, bos_id, eos_id,
                        d_out_ids, ld_ids, d_out_logprob, ld_logprob, d_limit, stream);
}

// ---- a wave's options: each drops the captured step, which holds the former setting ----------------------------------------------------
extern "C" int kzv_stream_set_topk(kzv_model* m, int k, int32_t* d_alt_ids, float* d_alt_logprob, int64_t ld_alt, void* stream) {
    (void)stream;                                // nothing is launched: the steps that follow carry one more kernel
    KZV_TRY(wave_check(m, "stream_set_topk", "kzv_stream_begin"));
    if (m->sbeams) return kzv_fail(KZV_E_STATE, "stream_set_topk: the wave is a beam search (alternatives are greedy only)");
    if (k < 0 || k > 8) return kzv_fail(KZV_E_ARG, "stream_set_topk: k must be in 0..8 (got %d; 0 switches the alternatives off)", k);
    if (k && (!d_alt_ids || !d_alt_logprob)) return kzv_fail(KZV_E_ARG, "stream_set_topk: null result array");
    if (k && ld_alt < (int64_t)m->sst.max_len * k) return kzv_fail(KZV_E_ARG, "stream_set_topk: ld_alt %lld < max_len * k = %lld", (long long)ld_alt, (long long)m->sst.max_len * k);
    drop_stream_graph(m);
    StreamWaveOpts& o = m->sopt;
    o.topk = k; o.alt_ids = k ? d_alt_ids : nullptr; o.alt_lp = k ? d_alt_logprob : nullptr; o.ld_alt = k ? ld_alt : 0;
    return KZV_OK;
}

extern "C" int kzv_stream_set_nbest(kzv_model* m, int n_best, int64_t* d_ids, int64_t ld_ids, float* d_scores, int32_t* d_lengths, float* d_logprob,
                                    int64_t ld_logprob, void* stream) {
    (void)stream;                                // nothing is launched: kzv_stream_start zeroes the log-probability rows with the token rows
    KZV_TRY(wave_check(m, "stream_set_nbest", "kzv_stream_begin_beams"));
    if (!m->sbeams) return kzv_fail(KZV_E_ARG, "stream_set_nbest: the wave is greedy (an n-best list needs a beam search: kzv_stream_begin_beams)");
    kzv_stream_beam_state& st = m->sbst;
    if (n_best < 1 || n_best > st.num_beams) return kzv_fail(KZV_E_ARG, "stream_set_nbest: n_best %d outside 1..num_beams = %d", n_best, st.num_beams);
    if (!d_ids || !d_scores || !d_lengths) return kzv_fail(KZV_E_ARG, "stream_set_nbest: null ids / scores / lengths");
    if (ld_ids < st.max_len || (d_logprob && ld_logprob < st.max_len)) return kzv_fail(KZV_E_ARG, "stream_set_nbest: output rows shorter than max_len = %d", st.max_len);
    drop_stream_graph(m);
    st.run_lp = st.fin_lp = nullptr;
    if (d_logprob) {                             // the log-probability rows, laid out as the token rows are: [slots, num_beams, max_len]
        const size_t rows = (size_t)m->B * st.max_len;
        if (!reserve(m, m->snbest, 2 * rows * sizeof(float))) return kzv_fail(KZV_E_HIP, "stream_set_nbest: log-probability rows allocation");
        st.run_lp = m->snbest.as<float>(); st.fin_lp = st.run_lp + rows;
    }
    st.n_best = n_best; st.nbest_ids = d_ids; st.ld_nbest = ld_ids; st.nbest_scores = d_scores; st.nbest_len = d_lengths;
    st.nbest_logprob = d_logprob; st.ld_nbest_logprob = d_logprob ? ld_logprob : 0;
    return KZV_OK;
}

extern "C" int kzv_stream_set_controls(kzv_model* m, const kzv_logits_controls* c, void* stream) {
    KZV_TRY(wave_check(m, "stream_set_controls", "kzv_stream_begin / kzv_stream_begin_beams"));
    if (!c) return kzv_fail(KZV_E_ARG, "stream_set_controls: null controls");
    if (c->no_repeat_ngram_size < 0 || c->no_repeat_ngram_size > 8) return kzv_fail(KZV_E_ARG, "stream_set_controls: no_repeat_ngram_size %d outside 0..8", c->no_repeat_ngram_size);
    if (!(c->repetition_penalty > 0.f)) return kzv_fail(KZV_E_ARG, "stream_set_controls: repetition_penalty must be positive (got %g)", (double)c->repetition_penalty);
    if (c->min_length < 0) return kzv_fail(KZV_E_ARG, "stream_set_controls: min_length must not be negative");
    if (m->V > 64 * 256) return kzv_fail(KZV_E_ARG, "stream_set_controls: vocabulary %d beyond 16,384", m->V);
    const int words = (m->V + 31) / 32, eos = WaveRows(m).eos_id;
    bool any = false;
    if (c->suppress_mask) {
        if ((c->suppress_mask[eos >> 5] >> (eos & 31)) & 1u) return kzv_fail(KZV_E_ARG, "stream_set_controls: the mask suppresses EOS (%d): no line could end", eos);
        int left = m->V;                         // tokens the mask leaves (bits past the vocabulary do not count)
        for (int i = 0; i < words; ++i) left -= __builtin_popcount(c->suppress_mask[i] & (i == words - 1 && (m->V & 31) ? (1u << (m->V & 31)) - 1u : ~0u));
        any = left < m->V;
        // a beam step ranks 2 * num_beams continuations of num_beams rows: with one token left they do not exist
        if (m->sbeams && left < 2) return kzv_fail(KZV_E_ARG, "stream_set_controls: the mask leaves %d token(s), a beam wave needs at least 2", left);
    }
    drop_stream_graph(m);
    StreamWaveOpts& o = m->sopt;
    o.ctl = *c; o.ctl.suppress_mask = nullptr; o.mask_on = false;
    if (any) {                                   // a copy on the stream, no kernel: the steps that follow read it
        m->smask_h.assign(c->suppress_mask, c->suppress_mask + words);
        if (!reserve(m, m->smask, sizeof(uint32_t) * (size_t)words)) return kzv_fail(KZV_E_HIP, "stream_set_controls: mask allocation");
        if (hipMemcpyAsync(m->smask.as<uint32_t>(), m->smask_h.data(), sizeof(uint32_t) * (size_t)words, hipMemcpyHostToDevice, (hipStream_t)stream) != hipSuccess)
            return kzv_fail(KZV_E_HIP, "stream_set_controls: mask copy");
        o.mask_on = true;
    }
    o.ctl_on = any || c->no_repeat_ngram_size != 0 || c->repetition_penalty != 1.f || c->min_length != 0;
    return KZV_OK;
}

const char* kzv_ngram_lm_problem(const kzv_ngram_lm* lm, int vocab);      // lm_fusion.hip

extern "C" int kzv_stream_set_lm(kzv_model* m, const kzv_ngram_lm* lm, float weight, void* stream) {
    (void)stream;                                // nothing is launched: the steps that follow carry one more kernel
    KZV_TRY(wave_check(m, "stream_set_lm", "kzv_stream_begin / kzv_stream_begin_beams"));
    if (const char* why = kzv_ngram_lm_problem(lm, m->V)) return kzv_fail(KZV_E_ARG, "stream_set_lm: %s", why);
    if (!std::isfinite(weight)) return kzv_fail(KZV_E_ARG, "stream_set_lm: the weight must be finite (got %g)", (double)weight);
    drop_stream_graph(m);
    m->sopt.lm = *lm; m->sopt.lm_weight = weight;
    m->sopt.lm_on = weight != 0.f;
    return KZV_OK;
}

extern "C" int kzv_stream_set_prefix(kzv_model* m, const int64_t* d_prefix, int64_t ld_prefix, const int32_t* d_prefix_len, float* d_forced_logprob,
                                     int64_t ld_forced_logprob, void* stream) {
    (void)stream;                                // nothing is launched: the steps that follow carry one more kernel
    KZV_TRY(wave_check(m, "stream_set_prefix", "kzv_stream_begin / kzv_stream_begin_beams"));
    const int max_len = WaveRows(m).max_len;
    if (ld_prefix < 0) return kzv_fail(KZV_E_ARG, "stream_set_prefix: ld_prefix must not be negative");
    if (ld_prefix > 0 && (!d_prefix || !d_prefix_len)) return kzv_fail(KZV_E_ARG, "stream_set_prefix: null prefix / prefix_len table");
    if (1 + ld_prefix > (int64_t)max_len - 1)
        return kzv_fail(KZV_E_ARG, "stream_set_prefix: BOS + %lld forced tokens reach max_len - 1 = %d: no token would be generated", (long long)ld_prefix, max_len - 1);
    if (m->V > 64 * 256) return kzv_fail(KZV_E_ARG, "stream_set_prefix: vocabulary %d beyond 16,384", m->V);
    if (ld_prefix > 0 && d_forced_logprob && ld_forced_logprob < ld_prefix + 1)
        return kzv_fail(KZV_E_ARG, "stream_set_prefix: forced_logprob rows of %lld columns are shorter than BOS + the %lld prefix columns", (long long)ld_forced_logprob, (long long)ld_prefix);
    drop_stream_graph(m);
    StreamWaveOpts& o = m->sopt;
    o.pfx_on = ld_prefix > 0;
    o.pfx = o.pfx_on ? d_prefix : nullptr; o.pfx_ld = ld_prefix; o.pfx_len = o.pfx_on ? d_prefix_len : nullptr;
    o.pfx_lp = o.pfx_on ? d_forced_logprob : nullptr; o.pfx_lp_ld = o.pfx_lp ? ld_forced_logprob : 0;
    return KZV_OK;
}

// ---- the score chain of a step, between the vocabulary GEMM and what reads the rows ---------------------------------------------------
// the wave's controls (order: repetition penalty, n-gram ban, minimum length, suppression -- immaterial, see logits_process.hip)
static int stream_process(kzv_model* m, const WaveRows& w, hipStream_t s) {
    const StreamWaveOpts& o = m->sopt;
    kzv_logits_process_args a;
    fill_rows(a, m, w);
    a.ids = w.ids; a.ld_ids = w.ld_ids; a.eos_id = w.eos_id;
    a.no_repeat_ngram_size = o.ctl.no_repeat_ngram_size; a.repetition_penalty = o.ctl.repetition_penalty; a.min_length = o.ctl.min_length;
    a.suppress_mask = o.mask_on ? m->smask.as<uint32_t>() : nullptr;
    a.normalise = m->sbeams ? 1 : 0;
    return kzv_logits_process(&a, s);
}

// the wave's language model on the step's (processed) scores: the next node, on the same histories
static int stream_lm_fuse(kzv_model* m, const WaveRows& w, hipStream_t s) {
    kzv_lm_fuse_args a;
    fill_rows(a, m, w);
    a.ids = w.ids; a.ld_ids = w.ld_ids;
    a.weight = m->sopt.lm_weight; a.lm = &m->sopt.lm;
    return kzv_lm_fuse(&a, s);
}

// the wave's forced prefixes on the step's scores: the chain's last node before selection, on every slot's own image and step
static int stream_force_prefix(kzv_model* m, const WaveRows& w, hipStream_t s, bool normalised) {
    const StreamWaveOpts& o = m->sopt;
    kzv_force_prefix_args a;
    fill_rows(a, m, w);
    a.prefix = o.pfx; a.ld_prefix = o.pfx_ld; a.prefix_len = o.pfx_len;
    a.normalised = normalised ? 1 : 0;
    a.forced_logprob = o.pfx_lp; a.ld_forced_logprob = o.pfx_lp_ld;
    return kzv_force_prefix(&a, s);
}

extern "C" int kzv_stream_encode(kzv_model* m, const float* d_pixel_values, int n, int first, void* stream) {
    if (!m || !m->bound) return kzv_fail(KZV_E_STATE, "stream_encode: model not bound");
    if (!m->swave) return kzv_fail(KZV_E_STATE, "stream_encode: call kzv_stream_begin first");
    if (first < 0 || n < 1 || first + n > m->spool_images) return kzv_fail(KZV_E_ARG, "stream_encode: entries %d .. %d outside the pool of %d images", first, first + n - 1, m->spool_images);
    if ((size_t)m->Ld * 2 * m->spool_images * m->npa * m->Hd * sizeof(bf16_t) > m->spool.capacity()) return kzv_fail(KZV_E_STATE, "stream_encode: the image width changed since kzv_stream_begin");
    KZV_TRY(kzv_encode_images(m, d_pixel_values, n, stream));
    return kzv_cross_relayout_pool(m->crosskv, m->spool.as<bf16_t>(), n, m->npa, m->c.dec_heads, 2 * m->Ld, m->spool_images, first, (hipStream_t)stream);
}

extern "C" int kzv_stream_start(kzv_model* m, void* stream) {
    KZV_TRY(wave_check(m, "stream_start", "kzv_stream_begin"));
    return m->sbeams ? kzv_stream_beam_seat_first(&m->sbst, stream) : kzv_stream_seat_first(&m->sst, stream);
}

static int stream_step_body(kzv_model* m, hipStream_t s) {
    KzvDecodeFused a;
    const int nb = m->sbeams;
    const WaveRows w(m);
    const StreamWaveOpts& o = m->sopt;
    KZV_TRY(fused_common(m, a, stream_e4m3(m), "stream_step"));
    a.ckv = m->spool.as<bf16_t>(); a.plane2 = (int64_t)m->spool_images * m->npa * m->Hd;
    a.tokens = w.tokens; a.posids = w.posids;
    a.group = w.group; a.slot_image = w.slot_image; a.slot_t = w.slot_t;
    if (nb) a.rows = m->sbst.rows;               // a slot's workgroup serves its nb rows through the handle's first row table
    KZV_TRY(kzv_decode_fused_launch(a, s));
    KZV_TRY(vocab_logits(m, true, m->slogits, s));
    // neutral controls and no language model: nothing is added to the chain.  A beam wave with the language model on normalises through
    // the controls' node even when the controls are neutral: the fusion acts on log-probabilities
    // Forced prefixes come last (the prompt is subject to neither) and take the same route in a beam wave: a forced row is no logits row.
    const bool lm = o.lm_on, pfx = o.pfx_on;
    if (o.ctl_on || ((lm || pfx) && nb)) KZV_TRY(stream_process(m, w, s));
    if (lm) KZV_TRY(stream_lm_fuse(m, w, s));
    if (pfx) KZV_TRY(stream_force_prefix(m, w, s, nb != 0));
    if (o.ctl_on || lm || pfx) {
        if (nb) {                                // the rows are processed log-probabilities now: ranked without a second normalisation
            KZV_TRY(kzv_beam_rank_logprobs(m->slogits, m->V, m->sbst.run_scores, m->sbst.slots, nb, m->V, 2 * nb, m->stop_lp, m->stop_ix, s));
            return kzv_stream_beam_update_prefix(&m->sbst, m->stop_lp, m->stop_ix, pfx ? o.pfx_len : nullptr, s);
        }
    }
    if (!nb) {                                   // the alternatives read slot_image / slot_t before seating replaces them
        if (o.topk) KZV_TRY(kzv_stream_topk(&m->sst, m->slogits, m->V, o.topk, o.alt_ids, o.alt_lp, o.ld_alt, s));
        return kzv_stream_update(&m->sst, m->slogits, m->V, s);
    }
    KZV_TRY(kzv_beam_topk(m->slogits, m->V, m->sbst.run_scores, m->sbst.slots, nb, m->V, 2 * nb, m->stop_lp, m->stop_ix, s));
    return kzv_stream_beam_update(&m->sbst, m->stop_lp, m->stop_ix, s);
}

extern "C" int kzv_stream_step(kzv_model* m, int graph, void* stream) {
    KZV_TRY(wave_check(m, "stream_step", "kzv_stream_begin"));
    if (!stream_supported(m, m->sbeams ? m->sbeams : 1)) return kzv_fail(KZV_E_STATE, "stream_step: the geometry or the step mode changed since kzv_stream_begin");
    hipStream_t s = (hipStream_t)stream;
    if (!graph) return stream_step_body(m, s);
    if (!stream) return kzv_fail(KZV_E_ARG, "stream_step: graph replay needs a non-default stream (stream capture)");
    if (!m->sgraph) {                            // kzv_stream_begin dropped the last wave's: captured at the wave's first step
        KZV_TRY(capture_into(&m->sgraph, s, "stream_step", [&] { return stream_step_body(m, s); }));
    }
    if (hipGraphLaunch(m->sgraph, s) != hipSuccess) return kzv_fail(KZV_E_HIP, "stream_step: launch");
    return KZV_OK;
}

static int stream_poll(kzv_model* m, const char* who, int32_t* finished, int32_t* steps, int32_t* pad_tokens, void* stream) {
    KZV_TRY(wave_check(m, who, "kzv_stream_begin"));
    if (!finished || !steps) return kzv_fail(KZV_E_ARG, "%s: null result", who);
    int32_t c[4] = {0, 0, 0, 0};
    const int n = m->sbeams ? 4 : 3;
    if (hipMemcpyAsync(c, WaveRows(m).counters, sizeof(int32_t) * n, hipMemcpyDeviceToHost, (hipStream_t)stream) != hipSuccess ||
        hipStreamSynchronize((hipStream_t)stream) != hipSuccess)
        return kzv_fail(KZV_E_HIP, "%s: copy", who);
    *finished = c[1]; *steps = c[2];
    if (pad_tokens) *pad_tokens = c[3];
    return KZV_OK;
}

extern "C" int kzv_stream_poll(kzv_model* m, int32_t* finished, int32_t* steps, void* stream) {
    return stream_poll(m, "stream_poll", finished, steps, nullptr, stream);
}

extern "C" int kzv_stream_poll_beams(kzv_model* m, int32_t* finished, int32_t* steps, int32_t* pad_tokens, void* stream) {
    KZV_TRY(wave_check(m, "stream_poll_beams", "kzv_stream_begin"));
    if (!pad_tokens) return kzv_fail(KZV_E_ARG, "stream_poll_beams: null result");
    return stream_poll(m, "stream_poll_beams", finished, steps, pad_tokens, stream);
}
