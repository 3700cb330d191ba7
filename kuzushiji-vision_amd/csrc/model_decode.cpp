// KV-cached generation on the model handle (N1): the cache, the cross-attention K/V layout and the fragment-ordered weight pack, the
// three bodies of one decoder step (one launch; LayerNorm folded into the GEMMs; a launch per operation) and the graph replay of the
// lockstep step (kzv_decode_*).  Slot-refill decoding (kzv_stream_*) is model_stream.cpp, on the helpers model_internal.h declares.
#include "model_internal.h"

static int g_decode_one_launch = -1;           // -1: KZV_DECODE_ONE_LAUNCH (default 1)
int decode_one_launch_mode() {
    if (g_decode_one_launch < 0) g_decode_one_launch = kzv_env_int("KZV_DECODE_ONE_LAUNCH", 1) != 0;
    return g_decode_one_launch;
}
extern "C" int kzv_set_decode_one_launch(int on) {
    if (on < -1 || on > 1) return kzv_fail(KZV_E_ARG, "set_decode_one_launch: -1 (environment default), 0 or 1");
    g_decode_one_launch = on;
    return KZV_OK;
}
static bool decode_one_launch(const kzv_model* m) {
    return decode_one_launch_mode() && m->Be >= 1 && m->B % m->Be == 0 && kzv_decode_fused_supported(m->Hd, m->c.dec_heads, m->Fd, m->Ld, m->B / m->Be, m->T, m->npa);
}
extern "C" int kzv_decode_step_impl(const kzv_model* m) {
    if (!m || !m->bound) return kzv_fail(KZV_E_STATE, "decode_step_impl: model not bound");
    return decode_one_launch(m) ? 1 : 0;
}

// e4m3 decoder weights: only the one-launch step reads them, so every case that step does not take keeps bf16 whatever was asked for
extern "C" int kzv_set_decode_weights(kzv_model* m, int format) {
    if (!m) return kzv_fail(KZV_E_ARG, "set_decode_weights: null model");
    if (format != KZV_DECODE_WEIGHTS_BF16 && format != KZV_DECODE_WEIGHTS_E4M3) return kzv_fail(KZV_E_ARG, "set_decode_weights: format 0 (bf16) or 1 (e4m3), not %d", format);
    m->dec_weights = format;
    return KZV_OK;
}
extern "C" int kzv_get_decode_weights(const kzv_model* m) {
    if (!m) return kzv_fail(KZV_E_ARG, "get_decode_weights: null model");
    return m->dec_weights;
}
static bool decode_e4m3(const kzv_model* m) { return m->dec_weights == KZV_DECODE_WEIGHTS_E4M3 && decode_one_launch(m); }
extern "C" int kzv_decode_weights_impl(const kzv_model* m) {
    if (!m || !m->bound) return kzv_fail(KZV_E_STATE, "decode_weights_impl: model not bound");
    return decode_e4m3(m) ? KZV_DECODE_WEIGHTS_E4M3 : KZV_DECODE_WEIGHTS_BF16;
}

// `bytes` in one of the handle's buffers (false: the allocation failed); a buffer that moved drops the graphs that hold its old pointer
bool reserve(kzv_model* m, KzvDevBuf& buf, size_t bytes) {
    const KzvDevBuf::Result r = buf.reserve(bytes);
    if (r == KzvDevBuf::MOVED) drop_decode_graphs(m);
    return r != KzvDevBuf::FAILED;
}

int ensure_kv_cache(kzv_model* m) {
    if (m->kvc && m->kvB == m->B && m->kvT == m->T) return KZV_OK;
    // ONE cache [2*Ld][B][T][Hd]: beam steps re-parent rows through the row tables instead of copying into a second cache
    const size_t bytes = (size_t)2 * m->Ld * m->B * m->T * m->Hd * sizeof(bf16_t);
    if (!reserve(m, m->kvc, bytes)) return kzv_fail(KZV_E_HIP, "decode_step: KV cache allocation (%zu bytes)", bytes);
    for (int i = 0; i < 2; ++i) if (!reserve(m, m->rowtab[i], (size_t)m->B * m->T * sizeof(int))) return kzv_fail(KZV_E_HIP, "decode_step: row table allocation");
    m->kvB = m->B; m->kvT = m->T; m->rt_cur = -1;
    drop_decode_graphs(m);           // a captured step holds B and T as well: dropped even where every block was large enough
    return KZV_OK;
}

// the decode-layout copy of the cross-attention K/V of the images encoded last (once per generation)
static int ensure_cross_layout(kzv_model* m, hipStream_t s) {
    if (m->ckv_dec_ok) return KZV_OK;
    const size_t bytes = (size_t)m->Ld * 2 * m->Be * m->npa * m->Hd * sizeof(bf16_t);
    if (!reserve(m, m->ckv_dec, bytes)) return kzv_fail(KZV_E_HIP, "decode: cross K/V copy allocation (%zu bytes)", bytes);
    KZV_TRY(kzv_cross_relayout(m->crosskv, m->ckv_dec.as<bf16_t>(), m->Be, m->npa, m->c.dec_heads, 2 * m->Ld, s));
    m->ckv_dec_ok = true;
    return KZV_OK;
}

// fragment-ordered copies of the decoder's weights (9.6 MB; layout: DecPack) for the one-launch generation step and the training forward's
// linear chains: ONE table-driven launch after every weight change (outside any capture)
bool dec_pack_wanted(const kzv_model* m) {
    return m->Hd == 256 && m->c.dec_heads == 4 && m->Fd == 768 && m->Ld >= 1 && m->Ld <= KZV_DECODE_FUSED_MAX_LAYERS;
}
int ensure_dec_pack(kzv_model* m, hipStream_t s) {
    if (m->dec_pack_ok || !dec_pack_wanted(m)) return KZV_OK;
    const DecPack& pk = m->pk;
    const int Hd = m->Hd;
    if (!reserve(m, m->dec_pack, sizeof(bf16_t) * (size_t)pk.total())) return kzv_fail(KZV_E_HIP, "decode: weight pack allocation");
    bf16_t* const base = m->dec_pack.as<bf16_t>();
    static const DecPack::Which six[6] = {DecPack::QKV, DecPack::O, DecPack::CQ, DecPack::CO, DecPack::FC1, DecPack::FC2};
    std::vector<KzvPackJob> jobs;
    for (int i = 0; i < m->Ld; ++i) {
        const DecLayerP& d = m->dp[i];
        const Lin* lin[6] = {&d.qkv, &d.o, &d.cq, &d.co, &d.fc1, &d.fc2};
        for (int j = 0; j < 6; ++j) jobs.push_back({lin[j]->h.w, base + pk.fwd(i, six[j]), lin[j]->N, lin[j]->K});
    }
    jobs.push_back({m->hd.h.w, base + pk.head_dense(), Hd, Hd});
    // the tied LM-head weight in 256-row chunks, zero rows beyond the vocabulary (head_ce_kernel)
    jobs.push_back({m->word.h.w, base + pk.head(), pk.vq, Hd, m->V});
    // the TRANSPOSED copies (B operands of the input-gradient GEMMs, kzv_dec_lin): [in, out] row-major, dense because out % 64 == 0
    for (int i = 0; i < m->Ld; ++i) {
        const DecLayerP& d = m->dp[i];
        const Lin* lin[6] = {&d.qkv, &d.o, &d.cq, &d.co, &d.fc1, &d.fc2};
        for (int j = 0; j < 6; ++j) jobs.push_back({lin[j]->h.wt, base + pk.tr(i, six[j]), lin[j]->K, lin[j]->N});
    }
    jobs.push_back({m->hd.h.wt, base + pk.head_dense_t(), Hd, Hd});
    // the tied LM-head weight transposed ([hidden, vocabulary]: the B operand of the head's input gradient inside head_ce_kernel), columns
    // beyond the padded vocabulary as zeros
    jobs.push_back({m->word.h.wt, base + pk.head_t(), Hd, pk.vq, Hd, (int)m->word.h.ldt, (int)m->Vp});
    KZV_TRY(kzv_pack_frag_multi(jobs.data(), (int)jobs.size(), s));      // frag_pack.hip: one launch for every matrix
    m->dec_pack_ok = true;
    return KZV_OK;
}

// the e4m3 stream and row scales of the same linears (4.7 MB), quantised from their bf16 copies in ONE launch (outside any capture)
int build_dec_pack8(kzv_model* m, hipStream_t s) {
    if (m->dec_pack8_ok) return KZV_OK;
    if (!reserve(m, m->dec_pack8, (size_t)kzv_decode_fused_pack8_bytes(m->Ld))) return kzv_fail(KZV_E_HIP, "decode: e4m3 weight stream allocation");
    if (!reserve(m, m->dec_scale8, sizeof(float) * (size_t)kzv_decode_fused_scales8(m->Ld))) return kzv_fail(KZV_E_HIP, "decode: e4m3 weight stream allocation");
    KzvDecodeFused8Src src[KZV_DECODE_FUSED_MAX_LAYERS];
    for (int i = 0; i < m->Ld; ++i) {
        const DecLayerP& d = m->dp[i];
        src[i] = KzvDecodeFused8Src{d.qkv.h.w, d.o.h.w, d.cq.h.w, d.co.h.w, d.fc1.h.w, d.fc2.h.w};
    }
    KZV_TRY(kzv_decode_fused_pack8(src, m->Ld, m->hd.h.w, m->dec_pack8.as<unsigned char>(), m->dec_scale8.as<float>(), s));
    m->dec_pack8_ok = true;
    return KZV_OK;
}
int ensure_dec_pack8(kzv_model* m, hipStream_t s) { return decode_e4m3(m) ? build_dec_pack8(m, s) : KZV_OK; }

// ---- one decoder step for the newest token of every sequence ------------------------------------------------------------------
// What every body gets: the step's operands; tptr != nullptr: the step index is read from device memory (graph replay), `t` is then
// only the host's copy for argument checks
struct StepArgs {
    const int64_t* tokens; const int* posids; int t; const int* tptr; const unsigned char* valid; int64_t ld_valid; float* logits;
};

// x = LayerNorm(x; gamma, beta), normalised by its consumer instead of being stored
struct LnSrc { const float* x = nullptr; const float* g = nullptr; const float* b = nullptr; };

// a generation-step GEMM whose A operand is LN(a) and / or whose RESID residual is LN(r) (hidden size 256: gemm_rows.hip); n: as LinOpts::n
static int lin_fwd_ln(const kzv_model* m, const Lin& l, const bf16_t* A, int64_t lda, int M, void* C, int64_t ldc, int epi, hipStream_t s,
                      const LnSrc& a_ln, const LnSrc& r_ln, void* aux = nullptr, int64_t ldaux = 0, int n = 0) {
    kzv_gemm_rows_ln_args a;
    memset(&a, 0, sizeof(a));
    a.A = A; a.lda = lda; a.B = l.h.w; a.ldb = l.K; a.C = C; a.ldc = ldc; a.bias = m->P + l.b; a.aux = aux; a.ldaux = ldaux;
    a.M = M; a.N = n ? n : l.N; a.K = l.K; a.n_valid = l.N;
    a.ln_a = a_ln.x; a.ln_a_gamma = a_ln.g; a.ln_a_beta = a_ln.b; a.ln_r = r_ln.x; a.ln_r_gamma = r_ln.g; a.ln_r_beta = r_ln.b; a.eps = m->c.ln_eps;
    return kzv_gemm_rows_ln(&a, epi, s);
}

// The vocabulary GEMM of a step: straight into the caller's [B, V] buffer where V % 4 == 0 (the padded scratch + copy costs a launch per
// token), else padded into m->logits and copied.  fold_ln: A = LN(hd_gelu) normalised inside the GEMM, else the stored m->hd_ln.
int vocab_logits(kzv_model* m, bool fold_ln, float* d_logits, hipStream_t s) {
    const bool direct = m->V % 4 == 0;
    float* C = direct ? d_logits : m->logits;
    const int n = direct ? m->V : m->Vp;
    if (fold_ln) KZV_TRY(lin_fwd_ln(m, m->word, nullptr, 0, m->B, C, n, KZV_EPI_F32, s, {m->hd_gelu, m->P + m->hln_w, m->P + m->hln_b}, {}, nullptr, 0, n));
    else KZV_TRY(lin_fwd(m, m->word, m->hd_ln, m->Hd, m->B, C, n, KZV_EPI_F32, s, {.n = n}));
    return direct ? KZV_OK : kzv_copy_logits(m->logits, m->Vp, d_logits, m->B, m->V, s);
}

// self-attention of the new token over the cache (appending its K/V at step t; cache rows: [head][T][64]) ...
static int self_attn_step(kzv_model* m, int i, const StepArgs& st, hipStream_t s) {
    const DecAct& a = m->da[i];
    const int B = m->B, Hd = m->Hd, T = m->T;
    bf16_t* cache = m->kvc.as<bf16_t>();
    const int64_t plane = (int64_t)B * T * Hd;  // one layer's K (or V) cache
    return kzv_attn_decode(a.qkv, 3 * Hd, a.qkv + Hd, a.qkv + 2 * Hd, 3 * Hd, cache + (int64_t)(2 * i) * plane, cache + (int64_t)(2 * i + 1) * plane,
                           (int64_t)T * Hd, 64, st.valid, st.ld_valid, a.ctx, Hd, B, m->c.dec_heads, st.tptr ? T : st.t + 1, st.t, s, st.tptr, 1,
                           m->rt_cur >= 0 ? m->rowtab[m->rt_cur].as<int>() : nullptr, T, (int64_t)T * 64);
}
// ... and cross-attention over the image's keys ([layer][K|V][image][head][key][64]; B / Be sequences share an image)
static int cross_attn_step(kzv_model* m, int i, hipStream_t s) {
    const DecAct& a = m->da[i];
    const int64_t img = (int64_t)m->npa * m->Hd, plane2 = (int64_t)m->Be * img;
    return kzv_attn_decode(a.cq, m->Hd, nullptr, nullptr, 0, m->ckv_dec.as<bf16_t>() + (int64_t)(2 * i) * plane2, m->ckv_dec.as<bf16_t>() + (int64_t)(2 * i + 1) * plane2,
                           img, 64, nullptr, 0, a.cctx, m->Hd, m->B, m->c.dec_heads, m->npa, -1, s, nullptr, m->B / m->Be, nullptr, 0, (int64_t)m->npa * 64);
}

// Hidden size 256: no LayerNorm launch at all -- each sub-layer output (fp32) stays un-normalised in memory and its two consumers
// (one GEMM's A operand, one later residual add) normalise it themselves (gemm_rows_ln_kernel).  20 launches fewer per token.
static int decode_step_body_fused(kzv_model* m, const StepArgs& st, hipStream_t s) {
    const int B = m->B, Hd = m->Hd, Fd = m->Fd;
    float* P = m->P;
    KZV_TRY(kzv_embed_gather(st.tokens, 1, st.posids, P + m->word.w, P + m->dtype, P + m->dpos, m->emb_sum, B, 1, Hd, s));
    LnSrc x{m->emb_sum, P + m->eln_w, P + m->eln_b};       // the layer's input, never stored
    for (int i = 0; i < m->Ld; ++i) {
        DecAct& a = m->da[i];
        const DecLayerP& d = m->dp[i];
        const LnSrc x1{a.s1, P + d.ln1w, P + d.ln1b}, x2{a.s2, P + d.ln2w, P + d.ln2b};
        KZV_TRY(lin_fwd_ln(m, d.qkv, nullptr, 0, B, a.qkv, 3 * Hd, KZV_EPI_BF16, s, x, {}));
        KZV_TRY(self_attn_step(m, i, st, s));
        KZV_TRY(lin_fwd_ln(m, d.o, a.ctx, Hd, B, a.s1, Hd, KZV_EPI_RESID, s, {}, x));
        KZV_TRY(lin_fwd_ln(m, d.cq, nullptr, 0, B, a.cq, Hd, KZV_EPI_BF16, s, x1, {}));
        KZV_TRY(cross_attn_step(m, i, s));
        KZV_TRY(lin_fwd_ln(m, d.co, a.cctx, Hd, B, a.s2, Hd, KZV_EPI_RESID, s, {}, x1));
        KZV_TRY(lin_fwd_ln(m, d.fc1, nullptr, 0, B, a.act, Fd, KZV_EPI_GELU, s, x2, {}, a.pre, Fd));
        KZV_TRY(lin_fwd_ln(m, d.fc2, a.act, Fd, B, a.s3, Hd, KZV_EPI_RESID, s, {}, x2));
        x = LnSrc{a.s3, P + d.ln3w, P + d.ln3b};
    }
    KZV_TRY(lin_fwd_ln(m, m->hd, nullptr, 0, B, m->hd_gelu, Hd, KZV_EPI_GELU_F32, s, x, {}, m->hd_pre, Hd));
    return vocab_logits(m, true, st.logits, s);
}

// The whole step up to the LM head's dense layer in ONE launch (decode_fused.hip: a workgroup per image owns its beams through all
// layers), then the vocabulary GEMM with the head's LayerNorm folded into its A operand as before.
// what every one-launch step reads whatever it serves: the weights in fragment order (or the e4m3 stream), embeddings, head, cache
int fused_common(kzv_model* m, KzvDecodeFused& a, bool e4m3, const char* who) {
    const int B = m->B, Hd = m->Hd, T = m->T;
    float* P = m->P;
    memset(&a, 0, sizeof(a));
    if (!m->dec_pack_ok) return kzv_fail(KZV_E_STATE, "%s: the fragment-ordered decoder weights are stale", who);
    const DecPack& pk = m->pk;
    const bf16_t* wp = m->dec_pack.as<bf16_t>();
    for (int i = 0; i < m->Ld; ++i) {
        const DecLayerP& d = m->dp[i];
        a.layers[i] = KzvDecodeFusedLayer{wp + pk.fwd(i, DecPack::QKV), wp + pk.fwd(i, DecPack::O), wp + pk.fwd(i, DecPack::CQ), wp + pk.fwd(i, DecPack::CO),
                                          wp + pk.fwd(i, DecPack::FC1), wp + pk.fwd(i, DecPack::FC2),
                                          P + d.qkv.b, P + d.o.b, P + d.cq.b, P + d.co.b, P + d.fc1.b, P + d.fc2.b,
                                          P + d.ln1w, P + d.ln1b, P + d.ln2w, P + d.ln2b, P + d.ln3w, P + d.ln3b};
    }
    a.nlayers = m->Ld;
    a.word = P + m->word.w; a.type0 = P + m->dtype; a.postab = P + m->dpos; a.elnw = P + m->eln_w; a.elnb = P + m->eln_b;
    a.whd = wp + pk.head_dense(); a.bhd = P + m->hd.b; a.hd_out = m->hd_gelu;
    a.cache = m->kvc.as<bf16_t>(); a.plane = (int64_t)B * T * Hd;
    a.T = T; a.npa = m->npa; a.B = B; a.eps = m->c.ln_eps;
    if (e4m3) {
        if (!m->dec_pack8_ok) return kzv_fail(KZV_E_STATE, "%s: the e4m3 decoder weights are stale", who);
        a.w8 = m->dec_pack8.as<unsigned char>(); a.scales8 = m->dec_scale8.as<float>();
    }
    return KZV_OK;
}

static int decode_step_body_one_launch(kzv_model* m, const StepArgs& st, hipStream_t s) {
    KzvDecodeFused a;
    KZV_TRY(fused_common(m, a, decode_e4m3(m), "decode_step"));
    a.tokens = st.tokens; a.posids = st.posids;
    a.ckv = m->ckv_dec.as<bf16_t>(); a.plane2 = (int64_t)m->Be * m->npa * m->Hd;
    a.valid = st.valid; a.ldvalid = st.ld_valid; a.tptr = st.tptr; a.t = st.t; a.group = m->B / m->Be;
    a.rows = m->rt_cur >= 0 ? m->rowtab[m->rt_cur].as<int>() : nullptr;
    KZV_TRY(kzv_decode_fused_launch(a, s));
    return vocab_logits(m, true, st.logits, s);
}

// a decoder sub-layer's output GEMM (residual add in its epilogue) and the LayerNorm after it.  (Fusing the two for N = 256 -- one
// 16-wave workgroup per 16 rows, wave w finishing row w -- was built and measured in round 2: bit-identical, and 100 us per step SLOWER:
// 16..64 large workgroups lose more to launch and single-CU load paths than the 19 saved ~5-us LayerNorm launches return.)
static int lin_resid_ln(kzv_model* m, const Lin& l, const bf16_t* A, const float* resid, float* sum, int64_t gw, int64_t gb, bf16_t* y16, float* y32,
                        float* stats, hipStream_t s) {
    KZV_TRY(lin_fwd(m, l, A, l.K, m->B, sum, l.N, KZV_EPI_RESID, s, {.resid = resid}));
    return ln_fwd(m, sum, gw, gb, y16, y32, stats, m->B, l.N, s);
}

static int decode_step_body(kzv_model* m, const StepArgs& st, hipStream_t s) {
    const int B = m->B, Hd = m->Hd, Fd = m->Fd;
    float* P = m->P;
    static int fuse_ln = -1;
    if (fuse_ln < 0) fuse_ln = kzv_env_int("KZV_DECODE_FUSE_LN", 1);
    if (decode_one_launch(m)) return decode_step_body_one_launch(m, st, s);
    if (fuse_ln && Hd == 256 && B <= 4096) return decode_step_body_fused(m, st, s);
    KzvRowsScope rows_scope;                     // M = B rows: every GEMM of the step takes the few-rows kernel (gemm_rows.hip)
    // embeddings of the one new token per sequence (HF modeling_roberta.py:75-122; position ids from the caller)
    KZV_TRY(kzv_embed_gather(st.tokens, 1, st.posids, P + m->word.w, P + m->dtype, P + m->dpos, m->emb_sum, B, 1, Hd, s));
    KZV_TRY(ln_fwd(m, m->emb_sum, m->eln_w, m->eln_b, m->xd0h, m->xd0, m->emb_st, B, Hd, s));
    const float* x = m->xd0; const bf16_t* xh = m->xd0h;
    for (int i = 0; i < m->Ld; ++i) {
        DecAct& a = m->da[i];
        const DecLayerP& d = m->dp[i];
        KZV_TRY(lin_fwd(m, d.qkv, xh, Hd, B, a.qkv, 3 * Hd, KZV_EPI_BF16, s));
        KZV_TRY(self_attn_step(m, i, st, s));
        KZV_TRY(lin_resid_ln(m, d.o, a.ctx, x, a.s1, d.ln1w, d.ln1b, a.x1h, a.x1, a.st1, s));
        KZV_TRY(lin_fwd(m, d.cq, a.x1h, Hd, B, a.cq, Hd, KZV_EPI_BF16, s));
        KZV_TRY(cross_attn_step(m, i, s));
        KZV_TRY(lin_resid_ln(m, d.co, a.cctx, a.x1, a.s2, d.ln2w, d.ln2b, a.x2h, a.x2, a.st2, s));
        KZV_TRY(lin_fwd(m, d.fc1, a.x2h, Hd, B, a.act, Fd, KZV_EPI_GELU, s, {.aux = a.pre, .ldaux = Fd}));
        KZV_TRY(lin_resid_ln(m, d.fc2, a.act, a.x2, a.s3, d.ln3w, d.ln3b, a.x3h, a.x3, a.st3, s));
        x = a.x3; xh = a.x3h;
    }
    KZV_TRY(lin_fwd(m, m->hd, xh, Hd, B, m->hd_gelu, Hd, KZV_EPI_GELU_F32, s, {.aux = m->hd_pre, .ldaux = Hd}));
    KZV_TRY(ln_fwd(m, m->hd_gelu, m->hln_w, m->hln_b, m->hd_ln, nullptr, m->hd_st, B, Hd, s));
    return vocab_logits(m, false, st.logits, s);
}

static int decode_step_check(kzv_model* m, const void* a, const void* b, const void* c, const void* d, const char* who) {
    if (!m || !m->bound) return kzv_fail(KZV_E_STATE, "%s: model not bound", who);
    if (!m->have_enc) return kzv_fail(KZV_E_STATE, "%s: call kzv_forward_loss / kzv_encode_images on the images first", who);
    if (!a || !b || !c || !d) return kzv_fail(KZV_E_ARG, "%s: null operand", who);
    if (m->Be < 1 || m->B % m->Be) return kzv_fail(KZV_E_STATE, "%s: %d decoder rows are not a multiple of the %d encoded images", who, m->B, m->Be);
    return KZV_OK;
}

extern "C" int kzv_decode_step(kzv_model* m, const int64_t* d_tokens, const int* d_posids, int t, const unsigned char* d_valid,
                               int64_t ld_valid, float* d_logits, void* stream) {
    KZV_TRY(decode_step_check(m, d_tokens, d_posids, d_valid, d_logits, "decode_step"));
    if (t < 0 || t >= m->T) return kzv_fail(KZV_E_ARG, "decode_step: step outside 0..T-1");
    KZV_TRY(ensure_kv_cache(m));
    if (t == 0) m->rt_cur = -1;                 // a new generation: no beam has been re-parented yet
    KZV_TRY(ensure_cross_layout(m, (hipStream_t)stream));
    KZV_TRY(ensure_dec_pack(m, (hipStream_t)stream));
    KZV_TRY(ensure_dec_pack8(m, (hipStream_t)stream));
    m->train = false; m->have_fwd = false; m->have_dec = false;      // decoder activations are overwritten: no backward after this
    return decode_step_body(m, StepArgs{d_tokens, d_posids, t, nullptr, d_valid, ld_valid, d_logits}, (hipStream_t)stream);
}

extern "C" int kzv_decode_begin(kzv_model* m, void* stream) {
    if (!m || !m->bound) return kzv_fail(KZV_E_STATE, "decode_begin: model not bound");
    KZV_TRY(ensure_kv_cache(m));
    if (m->have_enc) KZV_TRY(ensure_cross_layout(m, (hipStream_t)stream));
    KZV_TRY(ensure_dec_pack(m, (hipStream_t)stream));
    KZV_TRY(ensure_dec_pack8(m, (hipStream_t)stream));
    m->rt_cur = -1;                              // a new generation: every sequence reads its own cache row
    if (hipMemsetAsync(m->d_t, 0, sizeof(int), (hipStream_t)stream) != hipSuccess) return kzv_fail(KZV_E_HIP, "decode_begin: memset");
    return KZV_OK;
}

extern "C" int kzv_decode_step_graph(kzv_model* m, const int64_t* d_tokens, const int* d_posids, const unsigned char* d_valid, int64_t ld_valid,
                                     float* d_logits, void* stream) {
    KZV_TRY(decode_step_check(m, d_tokens, d_posids, d_valid, d_logits, "decode_step_graph"));
    if (!stream) return kzv_fail(KZV_E_ARG, "decode_step_graph: needs a non-default stream (stream capture)");
    KZV_TRY(ensure_kv_cache(m));
    KZV_TRY(ensure_cross_layout(m, (hipStream_t)stream));          // before any capture: a plain launch, once per generation
    KZV_TRY(ensure_dec_pack(m, (hipStream_t)stream));
    KZV_TRY(ensure_dec_pack8(m, (hipStream_t)stream));
    m->train = false; m->have_fwd = false; m->have_dec = false;
    hipStream_t s = (hipStream_t)stream;
    const int g = m->rt_cur + 1;
    const void* key[6] = {d_tokens, d_posids, d_valid, d_logits, m->kvc.as<void>(), (const void*)((intptr_t)m->ckv_dec.as<void>() ^ (intptr_t)(m->npa * 4096 + m->Be) ^ ((intptr_t)decode_one_launch_mode() << 40) ^ ((intptr_t)decode_e4m3(m) << 41))};
    bool same = m->dgraph[g] != nullptr && m->dg_ld[g] == ld_valid;
    for (int i = 0; i < 6 && same; ++i) same = m->dg_key[g][i] == key[i];
    if (!same) {                               // (re)capture: the step with its index read from m->d_t, then t += 1
        if (m->dgraph[g]) { (void)hipGraphExecDestroy(m->dgraph[g]); m->dgraph[g] = nullptr; }
        KZV_TRY(capture_into(&m->dgraph[g], s, "decode_step_graph", [&] {
            KZV_TRY(decode_step_body(m, StepArgs{d_tokens, d_posids, 0, m->d_t, d_valid, ld_valid, d_logits}, s));
            return kzv_step_inc(m->d_t, s);
        }));
        for (int i = 0; i < 6; ++i) m->dg_key[g][i] = key[i];
        m->dg_ld[g] = ld_valid;
    }
    if (hipGraphLaunch(m->dgraph[g], s) != hipSuccess) return kzv_fail(KZV_E_HIP, "decode_step_graph: launch");
    return KZV_OK;
}

extern "C" int kzv_decode_reorder(kzv_model* m, const int64_t* d_rows, int len, void* stream) {
    if (!m || !m->bound || !m->kvc) return kzv_fail(KZV_E_STATE, "decode_reorder: no KV cache (call kzv_decode_step first)");
    if (!d_rows || len < 1 || len > m->T) return kzv_fail(KZV_E_ARG, "decode_reorder: rows / length");
    // no cache row moves: the next step's attention reads key j of sequence b from the row of the ancestor that wrote it
    const int nxt = m->rt_cur < 0 ? 0 : m->rt_cur ^ 1;
    KZV_TRY(kzv_kv_rows(m->rt_cur < 0 ? nullptr : m->rowtab[m->rt_cur].as<int>(), m->rowtab[nxt].as<int>(), d_rows, m->B, m->T, len, (hipStream_t)stream));
    m->rt_cur = nxt;
    return KZV_OK;
}
