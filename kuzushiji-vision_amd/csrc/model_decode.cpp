// KV-cached generation on the model handle (N1): the cache, the cross-attention K/V layout and the fragment-ordered weight pack, the
// three bodies of one decoder step (one launch; LayerNorm folded into the GEMMs; a launch per operation) and the graph replay.
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
static bool reserve(kzv_model* m, KzvDevBuf& buf, size_t bytes) {
    const KzvDevBuf::Result r = buf.reserve(bytes);
    if (r == KzvDevBuf::MOVED) drop_decode_graphs(m);
    return r != KzvDevBuf::FAILED;
}

static int ensure_kv_cache(kzv_model* m) {
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
static int build_dec_pack8(kzv_model* m, hipStream_t s) {
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
static int vocab_logits(kzv_model* m, bool fold_ln, float* d_logits, hipStream_t s) {
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
static int fused_common(kzv_model* m, KzvDecodeFused& a, bool e4m3, const char* who) {
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

// Captures what `body` launches on `s` into an instantiated graph: the capture is ended and the graph destroyed on every path; the
// body's error comes back as it is, a failure of the capture itself as KZV_E_HIP
template <typename Body>
static int capture_into(hipGraphExec_t* out, hipStream_t s, const char* what, Body&& body) {
    if (hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal) != hipSuccess) return kzv_fail(KZV_E_HIP, "%s: begin capture", what);
    const int rc = body();
    hipGraph_t graph = nullptr;
    const hipError_t e = hipStreamEndCapture(s, &graph);
    if (rc != KZV_OK) { if (graph) (void)hipGraphDestroy(graph); return rc; }
    if (e != hipSuccess || !graph) return kzv_fail(KZV_E_HIP, "%s: end capture (%s)", what, hipGetErrorString(e));
    const hipError_t ei = hipGraphInstantiate(out, graph, nullptr, nullptr, 0);
    (void)hipGraphDestroy(graph);
    if (ei != hipSuccess) { *out = nullptr; return kzv_fail(KZV_E_HIP, "%s: instantiate (%s)", what, hipGetErrorString(ei)); }
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

// ---- slot-refill decoding (include/kzv.h: kzv_stream_*): greedy, one row per slot; or beam search, a slot holding an image's beam group ----
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
    if (m->sgraph) { (void)hipGraphExecDestroy(m->sgraph); m->sgraph = nullptr; }      // it holds the last wave's outputs and counts
    const size_t bytes = (size_t)m->Ld * 2 * pool_images * m->npa * m->Hd * sizeof(bf16_t);
    if (!reserve(m, m->spool, bytes)) return kzv_fail(KZV_E_HIP, "%s: pool allocation (%zu bytes)", who, bytes);
    m->spool_images = pool_images;
    // logits [B, V] | tokens [B] int64 | slot_image, slot_t, posids [B] | scratch [2 B] | counters [4]; a beam wave adds
    // run_seq, fin_seq [B, L] and fin_len [B] int64 | top_ix [2 B] int64 | run / fin scores [B], top_lp [2 B] | divisors [L + 1] | fin_done [B], unsat [B]
    const int L = m->L;
    const size_t sb = align_up((size_t)B * V * sizeof(float), 256) + (size_t)B * 8 + (size_t)B * 5 * 4 + 16 +
                      (nb > 1 ? (size_t)B * (2 * L + 1 + 2) * 8 + (size_t)B * 4 * 4 + align_up((size_t)(L + 1) * 4, 8) + (size_t)B * 2 : 0);
    if (!m->sstate || m->sstate_slots < B || m->sstate_V < V || m->sstate.capacity() < sb) {
        if (!reserve(m, m->sstate, sb)) return kzv_fail(KZV_E_HIP, "%s: slot state allocation (%zu bytes)", who, sb);
        m->sstate_slots = B; m->sstate_V = V;
    }
    char* q = m->sstate.as<char>();
    m->slogits = (float*)q; q += align_up((size_t)B * V * sizeof(float), 256);
    m->sbeams = nb > 1 ? nb : 0;
    m->stopk = 0;                                // kzv_stream_set_topk belongs to one wave
    m->sctl_on = false; m->smask_on = false;     // and so does kzv_stream_set_controls (neutral until it is called)
    m->sctl = kzv_logits_controls{}; m->sctl.repetition_penalty = 1.f;
    m->slm_on = false;                           // and kzv_stream_set_lm
    m->spfx_on = false; m->spfx = nullptr; m->spfx_len = nullptr; m->spfx_lp = nullptr; m->spfx_ld = m->spfx_lp_ld = 0;      // and kzv_stream_set_prefix
    if (nb == 1) {
        kzv_stream_state& st = m->sst;
        st.slots = B; st.n_images = n_images; st.max_len = max_len; st.vocab = V; st.pad_id = m->c.pad_id; st.bos_id = bos_id; st.eos_id = eos_id; st.reserved = 0;
        st.tokens = (int64_t*)q; q += (size_t)B * 8;
        st.slot_image = (int32_t*)q; q += (size_t)B * 4;
        st.slot_t = (int32_t*)q; q += (size_t)B * 4;
        st.posids = (int32_t*)q; q += (size_t)B * 4;
        st.scratch = (int32_t*)q; q += (size_t)B * 8;
        st.counters = (int32_t*)q;
        st.out_ids = d_out_ids; st.ld_ids = ld_ids; st.out_logprob = d_out_logprob; st.ld_logprob = ld_logprob; st.limit = d_limit;
    } else {
        kzv_stream_beam_state& st = m->sbst;
        st.slots = slots; st.n_images = n_images; st.num_beams = nb; st.max_len = max_len; st.vocab = V; st.pad_id = m->c.pad_id; st.bos_id = bos_id;
        st.eos_id = eos_id; st.early_stopping = early ? 1 : 0;
        st.n_best = 0; st.run_lp = st.fin_lp = nullptr;      // kzv_stream_set_nbest belongs to one wave
        st.nbest_ids = nullptr; st.ld_nbest = 0; st.nbest_scores = nullptr; st.nbest_len = nullptr; st.nbest_logprob = nullptr; st.ld_nbest_logprob = 0;
        st.tokens = (int64_t*)q; q += (size_t)B * 8;                       // 8-byte words first
        st.run_seq = (int64_t*)q; q += (size_t)B * max_len * 8;
        st.fin_seq = (int64_t*)q; q += (size_t)B * max_len * 8;
        st.fin_len = (int64_t*)q; q += (size_t)B * 8;
        m->stop_ix = (int64_t*)q; q += (size_t)B * 2 * 8;
        st.run_scores = (float*)q; q += (size_t)B * 4;
        st.fin_scores = (float*)q; q += (size_t)B * 4;
        m->stop_lp = (float*)q; q += (size_t)B * 2 * 4;
        st.posids = (int32_t*)q; q += (size_t)B * 4;
        st.slot_image = (int32_t*)q; q += (size_t)slots * 4;
        st.slot_t = (int32_t*)q; q += (size_t)slots * 4;
        st.scratch = (int32_t*)q; q += (size_t)slots * 8;
        st.counters = (int32_t*)q; q += 16;
        float* div = (float*)q; q += align_up((size_t)(max_len + 1) * 4, 8);
        st.fin_done = (uint8_t*)q; q += (size_t)B;
        st.unsatisfied = (uint8_t*)q;
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

extern "C" int kzv_stream_set_topk(kzv_model* m, int k, int32_t* d_alt_ids, float* d_alt_logprob, int64_t ld_alt, void* stream) {
    (void)stream;                                // nothing is launched: the steps that follow carry one more kernel
    if (!m || !m->bound || !m->swave) return kzv_fail(KZV_E_STATE, "stream_set_topk: call kzv_stream_begin first");
    if (m->sbeams) return kzv_fail(KZV_E_STATE, "stream_set_topk: the wave is a beam search (alternatives are greedy only)");
    if (k < 0 || k > 8) return kzv_fail(KZV_E_ARG, "stream_set_topk: k must be in 0..8 (got %d; 0 switches the alternatives off)", k);
    if (k && (!d_alt_ids || !d_alt_logprob)) return kzv_fail(KZV_E_ARG, "stream_set_topk: null result array");
    if (k && ld_alt < (int64_t)m->sst.max_len * k) return kzv_fail(KZV_E_ARG, "stream_set_topk: ld_alt %lld < max_len * k = %lld", (long long)ld_alt, (long long)m->sst.max_len * k);
    if (m->sgraph) { (void)hipGraphExecDestroy(m->sgraph); m->sgraph = nullptr; }      // a captured step holds the former setting
    m->stopk = k; m->salt_ids = k ? d_alt_ids : nullptr; m->salt_lp = k ? d_alt_logprob : nullptr; m->sld_alt = k ? ld_alt : 0;
    return KZV_OK;
}

extern "C" int kzv_stream_set_nbest(kzv_model* m, int n_best, int64_t* d_ids, int64_t ld_ids, float* d_scores, int32_t* d_lengths, float* d_logprob,
                                    int64_t ld_logprob, void* stream) {
    (void)stream;                                // nothing is launched: kzv_stream_start zeroes the log-probability rows with the token rows
    if (!m || !m->bound || !m->swave) return kzv_fail(KZV_E_STATE, "stream_set_nbest: call kzv_stream_begin_beams first");
    if (!m->sbeams) return kzv_fail(KZV_E_ARG, "stream_set_nbest: the wave is greedy (an n-best list needs a beam search: kzv_stream_begin_beams)");
    kzv_stream_beam_state& st = m->sbst;
    if (n_best < 1 || n_best > st.num_beams) return kzv_fail(KZV_E_ARG, "stream_set_nbest: n_best %d outside 1..num_beams = %d", n_best, st.num_beams);
    if (!d_ids || !d_scores || !d_lengths) return kzv_fail(KZV_E_ARG, "stream_set_nbest: null ids / scores / lengths");
    if (ld_ids < st.max_len || (d_logprob && ld_logprob < st.max_len)) return kzv_fail(KZV_E_ARG, "stream_set_nbest: output rows shorter than max_len = %d", st.max_len);
    if (m->sgraph) { (void)hipGraphExecDestroy(m->sgraph); m->sgraph = nullptr; }      // a captured step holds the former setting
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
    if (!m || !m->bound || !m->swave) return kzv_fail(KZV_E_STATE, "stream_set_controls: call kzv_stream_begin / kzv_stream_begin_beams first");
    if (!c) return kzv_fail(KZV_E_ARG, "stream_set_controls: null controls");
    if (c->no_repeat_ngram_size < 0 || c->no_repeat_ngram_size > 8) return kzv_fail(KZV_E_ARG, "stream_set_controls: no_repeat_ngram_size %d outside 0..8", c->no_repeat_ngram_size);
    if (!(c->repetition_penalty > 0.f)) return kzv_fail(KZV_E_ARG, "stream_set_controls: repetition_penalty must be positive (got %g)", (double)c->repetition_penalty);
    if (c->min_length < 0) return kzv_fail(KZV_E_ARG, "stream_set_controls: min_length must not be negative");
    if (m->V > 64 * 256) return kzv_fail(KZV_E_ARG, "stream_set_controls: vocabulary %d beyond 16,384", m->V);
    const int words = (m->V + 31) / 32, eos = m->sbeams ? m->sbst.eos_id : m->sst.eos_id;
    bool any = false;
    if (c->suppress_mask) {
        if ((c->suppress_mask[eos >> 5] >> (eos & 31)) & 1u) return kzv_fail(KZV_E_ARG, "stream_set_controls: the mask suppresses EOS (%d): no line could end", eos);
        int left = m->V;                         // tokens the mask leaves (bits past the vocabulary do not count)
        for (int i = 0; i < words; ++i) left -= __builtin_popcount(c->suppress_mask[i] & (i == words - 1 && (m->V & 31) ? (1u << (m->V & 31)) - 1u : ~0u));
        any = left < m->V;
        // a beam step ranks 2 * num_beams continuations of num_beams rows: with one token left they do not exist
        if (m->sbeams && left < 2) return kzv_fail(KZV_E_ARG, "stream_set_controls: the mask leaves %d token(s), a beam wave needs at least 2", left);
    }
    if (m->sgraph) { (void)hipGraphExecDestroy(m->sgraph); m->sgraph = nullptr; }      // a captured step holds the former setting
    m->sctl = *c; m->sctl.suppress_mask = nullptr; m->smask_on = false;
    if (any) {                                   // a copy on the stream, no kernel: the steps that follow read it
        m->smask_h.assign(c->suppress_mask, c->suppress_mask + words);
        if (!reserve(m, m->smask, sizeof(uint32_t) * (size_t)words)) return kzv_fail(KZV_E_HIP, "stream_set_controls: mask allocation");
        if (hipMemcpyAsync(m->smask.as<uint32_t>(), m->smask_h.data(), sizeof(uint32_t) * (size_t)words, hipMemcpyHostToDevice, (hipStream_t)stream) != hipSuccess)
            return kzv_fail(KZV_E_HIP, "stream_set_controls: mask copy");
        m->smask_on = true;
    }
    m->sctl_on = any || c->no_repeat_ngram_size != 0 || c->repetition_penalty != 1.f || c->min_length != 0;
    return KZV_OK;
}

const char* kzv_ngram_lm_problem(const kzv_ngram_lm* lm, int vocab);      // lm_fusion.hip

extern "C" int kzv_stream_set_lm(kzv_model* m, const kzv_ngram_lm* lm, float weight, void* stream) {
    (void)stream;                                // nothing is launched: the steps that follow carry one more kernel
    if (!m || !m->bound || !m->swave) return kzv_fail(KZV_E_STATE, "stream_set_lm: call kzv_stream_begin / kzv_stream_begin_beams first");
    if (const char* why = kzv_ngram_lm_problem(lm, m->V)) return kzv_fail(KZV_E_ARG, "stream_set_lm: %s", why);
    if (!std::isfinite(weight)) return kzv_fail(KZV_E_ARG, "stream_set_lm: the weight must be finite (got %g)", (double)weight);
    if (m->sgraph) { (void)hipGraphExecDestroy(m->sgraph); m->sgraph = nullptr; }      // a captured step holds the former setting
    m->slm = *lm; m->slm_weight = weight;
    m->slm_on = weight != 0.f;
    return KZV_OK;
}

extern "C" int kzv_stream_set_prefix(kzv_model* m, const int64_t* d_prefix, int64_t ld_prefix, const int32_t* d_prefix_len, float* d_forced_logprob,
                                     int64_t ld_forced_logprob, void* stream) {
    (void)stream;                                // nothing is launched: the steps that follow carry one more kernel
    if (!m || !m->bound || !m->swave) return kzv_fail(KZV_E_STATE, "stream_set_prefix: call kzv_stream_begin / kzv_stream_begin_beams first");
    const int max_len = m->sbeams ? m->sbst.max_len : m->sst.max_len;
    if (ld_prefix < 0) return kzv_fail(KZV_E_ARG, "stream_set_prefix: ld_prefix must not be negative");
    if (ld_prefix > 0 && (!d_prefix || !d_prefix_len)) return kzv_fail(KZV_E_ARG, "stream_set_prefix: null prefix / prefix_len table");
    if (1 + ld_prefix > (int64_t)max_len - 1)
        return kzv_fail(KZV_E_ARG, "stream_set_prefix: BOS + %lld forced tokens reach max_len - 1 = %d: no token would be generated", (long long)ld_prefix, max_len - 1);
    if (m->V > 64 * 256) return kzv_fail(KZV_E_ARG, "stream_set_prefix: vocabulary %d beyond 16,384", m->V);
    if (ld_prefix > 0 && d_forced_logprob && ld_forced_logprob < ld_prefix + 1)
        return kzv_fail(KZV_E_ARG, "stream_set_prefix: forced_logprob rows of %lld columns are shorter than BOS + the %lld prefix columns", (long long)ld_forced_logprob, (long long)ld_prefix);
    if (m->sgraph) { (void)hipGraphExecDestroy(m->sgraph); m->sgraph = nullptr; }      // a captured step holds the former setting
    m->spfx_on = ld_prefix > 0;
    m->spfx = m->spfx_on ? d_prefix : nullptr; m->spfx_ld = ld_prefix; m->spfx_len = m->spfx_on ? d_prefix_len : nullptr;
    m->spfx_lp = m->spfx_on ? d_forced_logprob : nullptr; m->spfx_lp_ld = m->spfx_lp ? ld_forced_logprob : 0;
    return KZV_OK;
}

// the wave's controls on the step's logits: one more node between the vocabulary GEMM and what reads the rows (order: repetition penalty,
// n-gram ban, minimum length, suppression -- immaterial, see logits_process.hip)
static int stream_process(kzv_model* m, hipStream_t s) {
    const int nb = m->sbeams;
    kzv_logits_process_args a;
    memset(&a, 0, sizeof(a));
    a.logits = m->slogits; a.ld = m->V; a.rows = m->B; a.vocab = m->V;
    if (!nb) { a.ids = m->sst.out_ids; a.ld_ids = m->sst.ld_ids; a.group = 1; a.slot_image = m->sst.slot_image; a.slot_t = m->sst.slot_t; a.by_image = 1; a.n_images = m->sst.n_images; a.eos_id = m->sst.eos_id; }
    else { a.ids = m->sbst.run_seq; a.ld_ids = m->sbst.max_len; a.group = nb; a.slot_image = m->sbst.slot_image; a.slot_t = m->sbst.slot_t; a.by_image = 0; a.n_images = m->sbst.n_images; a.eos_id = m->sbst.eos_id; }
    a.no_repeat_ngram_size = m->sctl.no_repeat_ngram_size; a.repetition_penalty = m->sctl.repetition_penalty; a.min_length = m->sctl.min_length;
    a.suppress_mask = m->smask_on ? m->smask.as<uint32_t>() : nullptr;
    a.normalise = nb ? 1 : 0;
    return kzv_logits_process(&a, s);
}

// the wave's language model on the step's (processed) scores: the next node, on the same histories
static int stream_lm_fuse(kzv_model* m, hipStream_t s) {
    const int nb = m->sbeams;
    kzv_lm_fuse_args a;
    memset(&a, 0, sizeof(a));
    a.logits = m->slogits; a.ld = m->V; a.rows = m->B; a.vocab = m->V;
    if (!nb) { a.ids = m->sst.out_ids; a.ld_ids = m->sst.ld_ids; a.group = 1; a.slot_image = m->sst.slot_image; a.slot_t = m->sst.slot_t; a.by_image = 1; a.n_images = m->sst.n_images; }
    else { a.ids = m->sbst.run_seq; a.ld_ids = m->sbst.max_len; a.group = nb; a.slot_image = m->sbst.slot_image; a.slot_t = m->sbst.slot_t; a.by_image = 0; a.n_images = m->sbst.n_images; }
    a.weight = m->slm_weight; a.lm = &m->slm;
    return kzv_lm_fuse(&a, s);
}

// the wave's forced prefixes on the step's scores: the chain's last node before selection, on every slot's own image and step
static int stream_force_prefix(kzv_model* m, hipStream_t s, bool normalised) {
    const int nb = m->sbeams;
    kzv_force_prefix_args a;
    memset(&a, 0, sizeof(a));
    a.logits = m->slogits; a.ld = m->V; a.rows = m->B; a.vocab = m->V;
    if (!nb) { a.group = 1; a.slot_image = m->sst.slot_image; a.slot_t = m->sst.slot_t; a.by_image = 1; a.n_images = m->sst.n_images; }
    else { a.group = nb; a.slot_image = m->sbst.slot_image; a.slot_t = m->sbst.slot_t; a.by_image = 0; a.n_images = m->sbst.n_images; }
    a.prefix = m->spfx; a.ld_prefix = m->spfx_ld; a.prefix_len = m->spfx_len;
    a.normalised = normalised ? 1 : 0;
    a.forced_logprob = m->spfx_lp; a.ld_forced_logprob = m->spfx_lp_ld;
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
    if (!m || !m->bound || !m->swave) return kzv_fail(KZV_E_STATE, "stream_start: call kzv_stream_begin first");
    return m->sbeams ? kzv_stream_beam_seat_first(&m->sbst, stream) : kzv_stream_seat_first(&m->sst, stream);
}

static int stream_step_body(kzv_model* m, hipStream_t s) {
    KzvDecodeFused a;
    const int nb = m->sbeams;
    KZV_TRY(fused_common(m, a, stream_e4m3(m), "stream_step"));
    a.ckv = m->spool.as<bf16_t>(); a.plane2 = (int64_t)m->spool_images * m->npa * m->Hd;
    if (!nb) {
        a.tokens = m->sst.tokens; a.posids = m->sst.posids;
        a.group = 1; a.slot_image = m->sst.slot_image; a.slot_t = m->sst.slot_t;
    } else {                                     // a slot's workgroup serves its nb rows through the handle's first row table
        a.tokens = m->sbst.tokens; a.posids = m->sbst.posids;
        a.group = nb; a.slot_image = m->sbst.slot_image; a.slot_t = m->sbst.slot_t; a.rows = m->sbst.rows;
    }
    KZV_TRY(kzv_decode_fused_launch(a, s));
    KZV_TRY(vocab_logits(m, true, m->slogits, s));
    // neutral controls and no language model: nothing is added to the chain.  A beam wave with the language model on normalises through
    // the controls' node even when the controls are neutral: the fusion acts on log-probabilities
    // Forced prefixes come last (the prompt is subject to neither) and take the same route in a beam wave: a forced row is no logits row.
    const bool lm = m->slm_on, pfx = m->spfx_on;
    if (m->sctl_on || ((lm || pfx) && nb)) KZV_TRY(stream_process(m, s));
    if (lm) KZV_TRY(stream_lm_fuse(m, s));
    if (pfx) KZV_TRY(stream_force_prefix(m, s, nb != 0));
    if (m->sctl_on || lm || pfx) {
        if (nb) {                                // the rows are processed log-probabilities now: ranked without a second normalisation
            KZV_TRY(kzv_beam_rank_logprobs(m->slogits, m->V, m->sbst.run_scores, m->sbst.slots, nb, m->V, 2 * nb, m->stop_lp, m->stop_ix, s));
            return kzv_stream_beam_update_prefix(&m->sbst, m->stop_lp, m->stop_ix, pfx ? m->spfx_len : nullptr, s);
        }
    }
    if (!nb) {                                   // the alternatives read slot_image / slot_t before seating replaces them
        if (m->stopk) KZV_TRY(kzv_stream_topk(&m->sst, m->slogits, m->V, m->stopk, m->salt_ids, m->salt_lp, m->sld_alt, s));
        return kzv_stream_update(&m->sst, m->slogits, m->V, s);
    }
    KZV_TRY(kzv_beam_topk(m->slogits, m->V, m->sbst.run_scores, m->sbst.slots, nb, m->V, 2 * nb, m->stop_lp, m->stop_ix, s));
    return kzv_stream_beam_update(&m->sbst, m->stop_lp, m->stop_ix, s);
}

extern "C" int kzv_stream_step(kzv_model* m, int graph, void* stream) {
    if (!m || !m->bound || !m->swave) return kzv_fail(KZV_E_STATE, "stream_step: call kzv_stream_begin first");
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
    if (!m || !m->bound || !m->swave) return kzv_fail(KZV_E_STATE, "%s: call kzv_stream_begin first", who);
    if (!finished || !steps) return kzv_fail(KZV_E_ARG, "%s: null result", who);
    int32_t c[4] = {0, 0, 0, 0};
    const int n = m->sbeams ? 4 : 3;
    if (hipMemcpyAsync(c, m->sbeams ? m->sbst.counters : m->sst.counters, sizeof(int32_t) * n, hipMemcpyDeviceToHost, (hipStream_t)stream) != hipSuccess ||
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
    if (m && m->bound && m->swave && !pad_tokens) return kzv_fail(KZV_E_ARG, "stream_poll_beams: null result");
    return stream_poll(m, "stream_poll_beams", finished, steps, pad_tokens, stream);
}
