// Forward / backward schedules of the TrOCR training step on the model handle.
//
// forward  = TrOCRModel.forward training branch (src/models/trocr_model.py:258-297):
//            ViTEncoder.forward (:169-202, 12 x HF ViTLayer pre-LN) -> encoder_decoder_proj (:269) ->
//            RobertaForCausalLM teacher-forced (HF modeling_roberta.py:75-122, 421-464, 877-893) -> CE (:292)
// backward = what loss.backward() does for that graph, hand-derived (no autograd), every matmul on the
//            MFMA GEMMs of gemm.hip, everything else fused into their epilogues or the HBM-bound kernels.
#include "model_internal.h"
#include <algorithm>
#include <cmath>
#include <optional>

// decoder_chain.hip: the linear chains of a decoder layer as two launches (KZV_DEC_CHAIN, kzv_set_dec_chain): 0 = off, 1 = the forward
// chains (+ the 256 x 256 input gradients on the row-panel kernel), 2 (default) = also the backward's row-local segments, one launch each
static int g_dec_chain = -1;
int dec_chain_mode() {
    if (g_dec_chain < 0) { g_dec_chain = kzv_env_int("KZV_DEC_CHAIN", 2); if (g_dec_chain < 0 || g_dec_chain > 2) g_dec_chain = 2; }
    return g_dec_chain;
}
extern "C" int kzv_set_dec_chain(int on) {
    if (on < -1 || on > 2) return kzv_fail(KZV_E_ARG, "set_dec_chain: -1 (environment default), 0, 1 or 2");
    g_dec_chain = on;
    return KZV_OK;
}
static int g_head_ce = -1;
bool head_ce_mode() {       // the one-launch LM head + CE (KZV_HEAD_CE / kzv_set_head_ce; default on)
    if (g_head_ce < 0) g_head_ce = kzv_env_int("KZV_HEAD_CE", 1) != 0;
    return g_head_ce != 0;
}
extern "C" int kzv_set_head_ce(int on) {
    if (on < -1 || on > 1) return kzv_fail(KZV_E_ARG, "set_head_ce: -1 (environment default), 0 or 1");
    g_head_ce = on;
    return KZV_OK;
}
// label smoothing of the training loss, per handle (F.cross_entropy(label_smoothing = eps)); evaluation forwards never apply it
extern "C" int kzv_set_label_smoothing(kzv_model* m, float eps) {
    if (!m) return kzv_fail(KZV_E_ARG, "set_label_smoothing: null model");
    if (!(eps >= 0.f && eps < 1.f)) return kzv_fail(KZV_E_ARG, "set_label_smoothing: %g is not in [0, 1)", (double)eps);
    if (eps > 0.f && m->focal_gamma > 0.f) return kzv_fail(KZV_E_ARG, "set_label_smoothing: %g with focal_gamma %g: no such loss is stated", (double)eps, (double)m->focal_gamma);
    m->label_smoothing = eps;
    return KZV_OK;
}
extern "C" float kzv_get_label_smoothing(const kzv_model* m) { return m ? m->label_smoothing : 0.f; }

// frozen bottom of the encoder, per handle: kzv_backward_segment skips the segments below the cut (embeddings and layers 0 .. n-1)
extern "C" int kzv_set_frozen_encoder_layers(kzv_model* m, int n) {
    if (!m) return kzv_fail(KZV_E_ARG, "set_frozen_encoder_layers: null model");
    if (n < 0 || n > m->Le) return kzv_fail(KZV_E_ARG, "set_frozen_encoder_layers: %d is not in 0..%d", n, m->Le);
    m->frozen_enc = n;
    return KZV_OK;
}
extern "C" int kzv_get_frozen_encoder_layers(const kzv_model* m) { return m ? m->frozen_enc : 0; }
// class weights and the focal exponent of the training loss, per handle (include/kzv.h); evaluation forwards never apply them
extern "C" int kzv_set_focal_gamma(kzv_model* m, float gamma) {
    if (!m) return kzv_fail(KZV_E_ARG, "set_focal_gamma: null model");
    if (!(gamma >= 0.f && gamma <= 5.f)) return kzv_fail(KZV_E_ARG, "set_focal_gamma: %g is not in [0, 5]", (double)gamma);
    if (gamma > 0.f && m->label_smoothing > 0.f) return kzv_fail(KZV_E_ARG, "set_focal_gamma: %g with label smoothing %g: no such loss is stated", (double)gamma, (double)m->label_smoothing);
    m->focal_gamma = gamma;
    return KZV_OK;
}
extern "C" float kzv_get_focal_gamma(const kzv_model* m) { return m ? m->focal_gamma : 0.f; }
extern "C" int kzv_set_class_weights(kzv_model* m, const float* host_weights, int n) {
    if (!m) return kzv_fail(KZV_E_ARG, "set_class_weights: null model");
    if (!host_weights && n == 0) { m->class_w_on = false; m->class_w_h.clear(); return KZV_OK; }
    if (!host_weights || n != m->c.vocab) return kzv_fail(KZV_E_ARG, "set_class_weights: %d weights, the vocabulary has %d", n, m->c.vocab);
    for (int i = 0; i < n; ++i)
        if (!(host_weights[i] > 0.f) || std::isinf(host_weights[i])) return kzv_fail(KZV_E_ARG, "set_class_weights: weight %d is %g (finite and > 0 wanted)", i, (double)host_weights[i]);
    // a forward in flight may still read the previous weights: wait for it, then copy (the caller's array may go away afterwards)
    if (hipDeviceSynchronize() != hipSuccess) return kzv_fail(KZV_E_HIP, "set_class_weights: synchronise");
    if (m->class_w.reserve(sizeof(float) * (size_t)n) == KzvDevBuf::FAILED) { m->class_w_on = false; m->class_w_h.clear(); return kzv_fail(KZV_E_HIP, "set_class_weights: allocation"); }
    if (hipMemcpy(m->class_w.as<float>(), host_weights, sizeof(float) * (size_t)n, hipMemcpyHostToDevice) != hipSuccess) {
        m->class_w_on = false; m->class_w_h.clear();
        return kzv_fail(KZV_E_HIP, "set_class_weights: copy");
    }
    m->class_w_h.assign(host_weights, host_weights + n);
    m->class_w_on = true;
    return KZV_OK;
}
extern "C" int kzv_get_class_weights(const kzv_model* m, float* host_out, int n) {
    if (!m || !m->class_w_on) return 0;
    const int have = (int)m->class_w_h.size();
    if (!host_out || n < have) return kzv_fail(KZV_E_ARG, "get_class_weights: room for %d weights, %d are set", n, have);
    std::copy(m->class_w_h.begin(), m->class_w_h.end(), host_out);
    return have;
}

namespace {

// ---- weight gradients -----------------------------------------------------------------------------------------------------
// dW[N, K] += dY[Mtok, N]^T . X[Mtok, K] (and dbias += column sums of dY) of one Linear
struct WgradOpts {
    bool bias = true;       // false: the bias gradient comes from elsewhere (a column-sum kernel) or the Linear's bias is not trained here
    int n = 0;              // the tied LM head only: dY padded to n columns, rows of dW beyond lin.N not stored
};
kzv_gemm_tn_args wgrad_args(const kzv_model* m, const Lin& l, const bf16_t* dY, int64_t ldy, const bf16_t* X, int64_t ldx, int Mtok, const WgradOpts& o) {
    kzv_gemm_tn_args a;
    memset(&a, 0, sizeof(a));
    a.P = dY; a.ldp = ldy; a.Q = X; a.ldq = ldx; a.OUT = m->G + l.w; a.ldo = l.K; a.Mtok = Mtok; a.N = o.n ? o.n : l.N; a.K = l.K; a.n_store = l.N;
    a.dbias = o.bias ? m->G + l.b : nullptr;
    return a;
}

int wgrad_flush(kzv_model* m, hipStream_t s) {
    if (m->wbatch.empty()) return KZV_OK;
    int rc = KZV_OK;
    for (size_t i = 0; i < m->wbatch.size() && rc == KZV_OK; i += 36)        // <= 36 problems per grid (gemm.hip TN_GROUP_MAX = 40)
        rc = kzv_gemm_tn_group(m->wbatch.data() + i, (int)std::min<size_t>(36, m->wbatch.size() - i), s);
    m->wbatch.clear();
    return rc;
}

// buffer classes whose last side-stream reader must finish before the main stream overwrites them
enum { CLS_DY = 0, CLS_DBIG = 1, CLS_DQKV = 2, CLS_MISC = 3 };

// on the side stream where it is in use (the event of `cls` marks the launch's end), else on `s`
int lin_wgrad(kzv_model* m, const Lin& l, int cls, hipStream_t s, const bf16_t* dY, int64_t ldy, const bf16_t* X, int64_t ldx, int Mtok,
              const WgradOpts& o = {}) {
    const kzv_gemm_tn_args a = wgrad_args(m, l, dY, ldy, X, ldx, Mtok, o);
    if (!m->use_side || (m->side_mode == 2 && !m->side_ok)) return kzv_gemm_tn(&a, s);
    if (hipEventRecord(m->ev_fork, s) != hipSuccess || hipStreamWaitEvent(m->side, m->ev_fork, 0) != hipSuccess)
        return kzv_fail(KZV_E_HIP, "wgrad_async: fork");
    const int rc = kzv_gemm_tn(&a, m->side);
    if (rc != KZV_OK) return rc;
    if (hipEventRecord(m->ev_done[cls], m->side) != hipSuccess) return kzv_fail(KZV_E_HIP, "wgrad_async: record");
    m->pending[cls] = true;
    return KZV_OK;
}
// Small weight gradients of one backward stage are collected and launched as ONE grid (wgrad_flush -> kzv_gemm_tn_group): each alone
// fills a fraction of the chip (4..12 tiles of 128x128).  Only without the side stream (which has its own overlap).
int lin_wgrad_batch(kzv_model* m, const Lin& l, int cls, hipStream_t s, const bf16_t* dY, int64_t ldy, const bf16_t* X, int64_t ldx, int Mtok,
                    const WgradOpts& o = {}) {
    if (m->use_side) return lin_wgrad(m, l, cls, s, dY, ldy, X, ldx, Mtok, o);
    m->wbatch.push_back(wgrad_args(m, l, dY, ldy, X, ldx, Mtok, o));
    return KZV_OK;
}
int wait_cls(kzv_model* m, int cls, hipStream_t s) {
    if (m->pending[cls]) {
        if (hipStreamWaitEvent(s, m->ev_done[cls], 0) != hipSuccess) return kzv_fail(KZV_E_HIP, "wait_cls");
        m->pending[cls] = false;
    }
    return KZV_OK;
}
int join_side(kzv_model* m, hipStream_t s) {
    for (int c = 0; c < 4; ++c) KZV_TRY(wait_cls(m, c, s));
    return KZV_OK;
}

// A Linear's input gradient (gemm_nt against the transposed weight, one-store epilogue) and weight gradient (gemm_tn) from the same dY:
// ONE launch when gemm_tn256.hip's pair kernel takes the shapes (kzv_gemm_pair_launch), else the two launches in the order the
// single-stream schedule has always issued them (weight gradient first).
int dgrad_wgrad(kzv_model* m, const Lin& l, int cls, hipStream_t s, const bf16_t* dY, int64_t ldy, int Mtok, void* dX, int64_t ldx, int epi,
                const bf16_t* X, int64_t ldxq, const LinOpts& o = {}) {
    // dX[Mtok, K] = dY[Mtok, N] . W[N, K]  (B operand = W^T copy [K, N]);  dW[N, K] += dY^T . X
    if (!m->use_side && !m->fp8) {
        kzv_gemm_nt_args na;
        memset(&na, 0, sizeof(na));
        na.A = dY; na.lda = ldy; na.B = l.h.wt; na.ldb = l.h.ldt; na.C = dX; na.ldc = ldx; na.ldr = ldx; na.aux = o.aux; na.ldaux = o.ldaux;
        na.M = Mtok; na.N = l.K; na.K = l.N; na.n_valid = l.K;
        const kzv_gemm_tn_args ta = wgrad_args(m, l, dY, ldy, X, ldxq, Mtok, {});
        const int rc = kzv_gemm_pair_launch(&na, epi, &ta, s);
        if (rc < 0) return kzv_fail(KZV_E_HIP, "dgrad_wgrad: pair launch");
        if (rc == 1) return KZV_OK;
    }
    KZV_TRY(lin_wgrad(m, l, cls, s, dY, ldy, X, ldxq, Mtok));
    return lin_dgrad(m, l, dY, ldy, Mtok, dX, ldx, epi, s, o);
}

// ---- attention sites ----------------------------------------------------------------------------------------------------
// One attention of the model: its operands in the saved activations, its geometry and its dropout site.  The forward launches it as it
// is; the backward adds the gradient pointers.
struct AttnSite {
    const bf16_t *Q, *K, *V; int64_t ldq, ldkv;
    bf16_t* O; int64_t ldo; float* LSE;
    int heads, head_dim, Sq, Sk, mode, batch;     // mode 1: causal + key padding from the labels
    float drop_p; uint32_t drop_key;
};
// cross-attention K (V = + Hd) of decoder layer i inside the all-layers projection [Mp, Ld * 2 * Hd], and their gradients
bf16_t* cross_kv(const kzv_model* m, int i) { return m->crosskv + (int64_t)i * 2 * m->Hd; }
bf16_t* cross_dkv(const kzv_model* m, int i) { return m->dckv + (int64_t)i * 2 * m->Hd; }

AttnSite enc_self(const kzv_model* m, int i, int batch) {
    const EncAct& a = m->ea[i];
    const int He = m->He;
    return {a.qkv, a.qkv + He, a.qkv + 2 * He, 3 * He, 3 * He, a.ctx, He, a.lse, m->c.enc_heads, He / m->c.enc_heads, m->Sa, m->Sa, 0, batch,
            dp(m, m->c.enc_attn_dropout), key(m, SITE_ENC_L + 4 * i)};
}
AttnSite dec_self(const kzv_model* m, int i) {
    const DecAct& a = m->da[i];
    const int Hd = m->Hd;
    return {a.qkv, a.qkv + Hd, a.qkv + 2 * Hd, 3 * Hd, 3 * Hd, a.ctx, Hd, a.lse_sa, m->c.dec_heads, 64, m->Ta, m->Ta, 1, m->B,
            dp(m, m->c.dec_attn_dropout), key(m, SITE_DEC_L + 8 * i)};
}
AttnSite dec_cross(const kzv_model* m, int i) {
    const DecAct& a = m->da[i];
    const int Hd = m->Hd;
    return {a.cq, cross_kv(m, i), cross_kv(m, i) + Hd, Hd, (int64_t)m->Ld * 2 * Hd, a.cctx, Hd, a.lse_ca, m->c.dec_heads, 64, m->Ta, m->npa, 0, m->B,
            dp(m, m->c.dec_attn_dropout), key(m, SITE_DEC_L + 8 * i + 2)};
}

int attn_launch(const kzv_model* m, const AttnSite& t, bool bwd, const bf16_t* dO, bf16_t* dQ, bf16_t* dK, bf16_t* dV, hipStream_t s) {
    kzv_attn_args a;
    memset(&a, 0, sizeof(a));
    a.Q = t.Q; a.K = t.K; a.V = t.V; a.O = t.O; a.LSE = t.LSE; a.dO = dO; a.dQ = dQ; a.dK = dK; a.dV = dV;
    a.ldq = t.ldq; a.ldk = t.ldkv; a.ldv = t.ldkv; a.ldo = t.ldo;
    a.ids = m->labels; a.ld_ids = m->L; a.pad_id = m->c.pad_id;
    a.B = t.batch; a.heads = t.heads; a.Sq = t.Sq; a.Sk = t.Sk; a.head_dim = t.head_dim; a.mode = t.mode; a.drop_p = t.drop_p; a.drop_key = t.drop_key;
    // decided (and validated) once; in a long-sequence model the key / query count alone picks the structure, per launch
    const int impl = kzv_attn_impl_ex(&a, bwd ? 1 : 0, m->long_seq ? KZV_MODEL_LONG_SEQ : 0);
    return impl < 0 ? impl : kzv_attn_launch(&a, impl, bwd, s);
}
int attn_fwd(const kzv_model* m, const AttnSite& t, hipStream_t s) { return attn_launch(m, t, false, nullptr, nullptr, nullptr, nullptr, s); }
int attn_bwd(const kzv_model* m, const AttnSite& t, const bf16_t* dO, bf16_t* dQ, bf16_t* dK, bf16_t* dV, hipStream_t s) {
    return attn_launch(m, t, true, dO, dQ, dK, dV, s);
}

// the decoder's packs exist and its geometry is the one the chain / segment / head kernels are built for
bool dec_packable(const kzv_model* m) { return dec_pack_wanted(m) && kzv_dec_chain_supported(m->Hd, m->Fd); }

}  // namespace

// ================================================================================================ forward
int forward(kzv_model* m, const float* px, const int64_t* labels, float* d_loss, float* d_logits, hipStream_t s,
            bool run_encoder, int logits_pos, int enc_batch, bool run_decoder) {
    const kzv_config& c = m->c;
    // T = ACTIVE decoder length (kzv_set_active_length): positions >= T hold only padding in every sample, are
    // masked as keys and carry no loss, so the decoder runs on the packed [B, T] prefix (rows b*T + t).
    const int T = m->Ta, He = m->He, Fe = m->Fe, Hd = m->Hd, Fd = m->Fd;
    int B = enc_batch > 0 ? enc_batch : m->B;          // encoder batch (kzv_encode_images: fewer images than decoder rows)
    const int Me = B * m->Sa, Mp = B * m->npa;
    float* P = m->P;
    const float eps = c.ln_eps;
    m->labels = labels;
    if (hipMemsetAsync(m->count, 0, 64 * sizeof(float), s) != hipSuccess) return kzv_fail(KZV_E_HIP, "forward: memset");
    const int CK = m->Ld * 2 * Hd;
    if (run_encoder) {
    // ---- patch embedding: Conv2d(k=s=16) == im2row + GEMM (trocr_model.py:77,89-90) -----------------
    KZV_TRY(kzv_im2row(px, m->patches, B, c.channels, c.image_h, m->img_w, c.patch_h, c.patch_w, s));
    KZV_TRY(lin_fwd(m, m->patch, m->patches, m->PD, Mp, m->pe32, He, KZV_EPI_F32, s));
    float* x0 = m->Le ? m->ea[0].x_in : m->x_last;
    KZV_TRY(kzv_embed_assemble(m->pe32, P + m->cls, P + m->pos, x0, B, m->npa, He, dp(m, c.enc_hidden_dropout), key(m, SITE_ENC_EMB), s,
                               m->img_w / c.patch_w, c.image_w / c.patch_w));
    // ---- ViT layers (pre-LN; HF modeling_vit.py:257-286) -----------------------------------------------
    const bool f8 = m->fp8 != 0;
    if (f8) KZV_TRY(kzv_fp8_roll(m->f8_q, m->f8_amax, m->f8_rows, m->Le, (int)m->f8_stride, s));
    // fp8 path: LayerNorm leaves an e4m3 copy of its output (one scale per row) for the GEMM behind it
    const LnFwdOpts ln8{.y8 = f8 ? m->x8 : nullptr, .y8_scale = f8 ? m->x8_scale : nullptr};
    const unsigned char* x8 = f8 ? m->x8 : nullptr;
    const float hp = dp(m, c.enc_hidden_dropout);
    for (int i = 0; i < m->Le; ++i) {
        EncAct& a = m->ea[i];
        const EncLayerP& e = m->ep[i];
        const uint32_t site = SITE_ENC_L + 4 * i;
        float* x_out = i + 1 < m->Le ? m->ea[i + 1].x_in : m->x_last;
        KZV_TRY(ln_fwd(m, a.x_in, e.ln1w, e.ln1b, a.ln1, nullptr, a.st1, Me, He, s, ln8));
        KZV_TRY(lin_fwd(m, e.qkv, a.ln1, He, Me, a.qkv, 3 * He, KZV_EPI_BF16, s, {.a8 = x8, .a8_scale = m->x8_scale}));
        KZV_TRY(attn_fwd(m, enc_self(m, i, B), s));
        KZV_TRY(lin_fwd(m, e.o, a.ctx, He, Me, a.x_mid, He, KZV_EPI_RESID, s, {.resid = a.x_in, .drop_p = hp, .drop_key = key(m, site + 1)}));
        KZV_TRY(ln_fwd(m, a.x_mid, e.ln2w, e.ln2b, a.ln2, nullptr, a.st2, Me, He, s, ln8));
        // fp8: the GELU epilogue also writes the e4m3 activation (per-tensor multiplier of this layer, amax for the next step's)
        KZV_TRY(lin_fwd(m, e.fc1, a.ln2, He, Me, a.act, Fe, KZV_EPI_GELU, s,
                        {.aux = a.pre, .ldaux = Fe, .a8 = x8, .a8_scale = m->x8_scale, .c8 = f8 ? m->act8 : nullptr, .c8_qscale = f8 ? m->f8_q + i : nullptr,
                         .c8_amax = f8 ? m->f8_amax + i : nullptr}));
        KZV_TRY(lin_fwd(m, e.fc2, a.act, Fe, Me, x_out, He, KZV_EPI_RESID, s,
                        {.resid = a.x_mid, .drop_p = hp, .drop_key = key(m, site + 2), .a8 = f8 ? m->act8 : nullptr,
                         .a8_scale = f8 ? m->f8_rows + (int64_t)i * m->f8_stride : nullptr}));
    }
    // final LN, drop CLS (trocr_model.py:197-200), projection (:269)
    KZV_TRY(ln_fwd(m, m->x_last, m->lnf_w, m->lnf_b, m->enc_out, nullptr, m->stf, Me, He, s, {.seq = m->Sa, .drop_first = 1}));
    if (m->has_proj) KZV_TRY(lin_fwd(m, m->proj, m->enc_out, He, Mp, m->proj_out, Hd, KZV_EPI_BF16, s));
    // cross-attention K/V of every decoder layer in one GEMM
    KZV_TRY(lin_fwd(m, m->ckv, m->proj_out, Hd, Mp, m->crosskv, CK, KZV_EPI_BF16, s));
    m->have_enc = true; m->Be = B; m->ckv_dec_ok = false;
    }   // run_encoder
    if (!run_decoder) return KZV_OK;
    B = m->B;
    if (m->Be != B) return kzv_fail(KZV_E_STATE, "forward: the encoder states hold %d images, the decoder batch is %d (kzv_encode_images is for kzv_decode_step only)", m->Be, B);
    const int Md = B * T;
    // ---- decoder embeddings (HF modeling_roberta.py:75-122,142-155) --------------------------------------
    KZV_TRY(kzv_dec_prepare(labels, B, m->L, T, c.pad_id, c.max_pos, m->posids, m->count, m->err, s));
    KZV_TRY(kzv_embed_gather(labels, m->L, m->posids, P + m->word.w, P + m->dtype, P + m->dpos, m->emb_sum, B, T, Hd, s));
    const float hp = dp(m, c.dec_hidden_dropout);
    KZV_TRY(ln_fwd(m, m->emb_sum, m->eln_w, m->eln_b, m->xd0h, m->xd0, m->emb_st, Md, Hd, s, {.drop_p = hp, .drop_key = key(m, SITE_DEC_EMB)}));
    // ---- decoder layers (post-LN; HF modeling_roberta.py:421-464) -------------------------------------------
    const float* x = m->xd0; const bf16_t* xh = m->xd0h;
    // the linear chains between the attentions as two launches per layer (decoder_chain.hip) where the geometry is the reference's
    const bool packable = dec_packable(m);
    const bool chain = dec_chain_mode() && packable;
    const bool fused_head = head_ce_mode() && packable && !d_logits;      // LM head + CE in one launch (below)
    if (chain || fused_head) KZV_TRY(ensure_dec_pack(m, s));
    const DecPack& pk = m->pk;
    for (int i = 0; i < m->Ld; ++i) {
        DecAct& a = m->da[i];
        const DecLayerP& d = m->dp[i];
        const uint32_t site = SITE_DEC_L + 8 * i;
        if (!chain || i == 0) KZV_TRY(lin_fwd(m, d.qkv, xh, Hd, Md, a.qkv, 3 * Hd, KZV_EPI_BF16, s));
        KZV_TRY(attn_fwd(m, dec_self(m, i), s));
        if (chain) {
            const bf16_t* wp = m->dec_pack.as<bf16_t>();
            // the fp32 LayerNorm outputs x1 / x2 / x3 feed nothing but the next residual add: the chains recompute them from the sums and
            // row statistics the backward needs anyway instead of writing and re-reading them (layer 0 adds the embedding output xd0)
            KzvDecChainA ca{a.ctx, i == 0 ? x : nullptr, wp + pk.fwd(i, DecPack::O), P + d.o.b, hp, key(m, site + 1), P + d.ln1w, P + d.ln1b,
                            wp + pk.fwd(i, DecPack::CQ), P + d.cq.b, a.s1, a.st1, nullptr, a.x1h, a.cq, Md, eps};
            if (i > 0) { const DecAct& pa = m->da[i - 1]; const DecLayerP& pd = m->dp[i - 1]; ca.xres_s = pa.s3; ca.xres_st = pa.st3; ca.xres_g = P + pd.ln3w; ca.xres_b = P + pd.ln3b; }
            KZV_TRY(kzv_dec_chain_a(ca, s));
        } else {
            KZV_TRY(lin_fwd(m, d.o, a.ctx, Hd, Md, a.s1, Hd, KZV_EPI_RESID, s, {.resid = x, .drop_p = hp, .drop_key = key(m, site + 1)}));
            KZV_TRY(ln_fwd(m, a.s1, d.ln1w, d.ln1b, a.x1h, a.x1, a.st1, Md, Hd, s));
            KZV_TRY(lin_fwd(m, d.cq, a.x1h, Hd, Md, a.cq, Hd, KZV_EPI_BF16, s));
        }
        KZV_TRY(attn_fwd(m, dec_cross(m, i), s));
        if (chain) {
            const bf16_t* wp = m->dec_pack.as<bf16_t>();
            const bool more = i + 1 < m->Ld;
            KzvDecChainB cb{a.cctx, nullptr, wp + pk.fwd(i, DecPack::CO), P + d.co.b, hp, key(m, site + 3), key(m, site + 4), P + d.ln2w, P + d.ln2b,
                            wp + pk.fwd(i, DecPack::FC1), P + d.fc1.b, wp + pk.fwd(i, DecPack::FC2), P + d.fc2.b, P + d.ln3w, P + d.ln3b,
                            more ? wp + pk.fwd(i + 1, DecPack::QKV) : nullptr, more ? P + m->dp[i + 1].qkv.b : nullptr,
                            a.s2, a.st2, nullptr, a.x2h, a.pre, a.act, a.s3, a.st3, nullptr, a.x3h, more ? m->da[i + 1].qkv : nullptr, Md, eps};
            cb.s1 = a.s1; cb.st1 = a.st1; cb.g1 = P + d.ln1w; cb.b1 = P + d.ln1b;
            KZV_TRY(kzv_dec_chain_b(cb, s));
        } else {
            KZV_TRY(lin_fwd(m, d.co, a.cctx, Hd, Md, a.s2, Hd, KZV_EPI_RESID, s, {.resid = a.x1, .drop_p = hp, .drop_key = key(m, site + 3)}));
            KZV_TRY(ln_fwd(m, a.s2, d.ln2w, d.ln2b, a.x2h, a.x2, a.st2, Md, Hd, s));
            KZV_TRY(lin_fwd(m, d.fc1, a.x2h, Hd, Md, a.act, Fd, KZV_EPI_GELU, s, {.aux = a.pre, .ldaux = Fd}));
            KZV_TRY(lin_fwd(m, d.fc2, a.act, Fd, Md, a.s3, Hd, KZV_EPI_RESID, s, {.resid = a.x2, .drop_p = hp, .drop_key = key(m, site + 4)}));
            KZV_TRY(ln_fwd(m, a.s3, d.ln3w, d.ln3b, a.x3h, a.x3, a.st3, Md, Hd, s));
        }
        x = a.x3; xh = a.x3h;
    }
    // ---- LM head (HF modeling_roberta.py:877-893; decoder.weight tied to word embeddings :684-687) + CE --------
    KZV_TRY(lin_fwd(m, m->hd, xh, Hd, Md, m->hd_gelu, Hd, KZV_EPI_GELU_F32, s, {.aux = m->hd_pre, .ldaux = Hd}));
    KZV_TRY(ln_fwd(m, m->hd_gelu, m->hln_w, m->hln_b, m->hd_ln, nullptr, m->hd_st, Md, Hd, s));
    // no logits asked for (the training / validation step): head GEMM + log-softmax + NLL + dlogits in ONE launch, the [B*T, Vp] fp32
    // logits never written (cross_entropy.hip head_ce_kernel).  Otherwise the GEMM materialises them and ce_kernel follows.
    const float ls_eps = m->train ? m->label_smoothing : 0.f;          // smoothing is a training criterion: validation logs the plain NLL
    // so are class weights and the focal term.  With either the normaliser is {W, S_w} at count + 4, summed in a fixed order
    const float* cls_w = m->train && m->class_w_on ? m->class_w.as<float>() : nullptr;
    const float focal = m->train ? m->focal_gamma : 0.f;
    const float* norm = m->count;
    if (cls_w || focal > 0.f) {
        KZV_TRY(kzv_target_weight_sum(labels, m->L, B, T, m->V, c.pad_id, cls_w, m->count + 4, s));
        norm = m->count + 4;
    }
    if (fused_head) {
        KzvHeadCE hc{m->hd_ln, m->dec_pack.as<bf16_t>() + pk.head(), P + m->word.b, labels, norm, m->loss_acc, m->train ? m->dlogits : nullptr, Md, m->L, T, m->V, (int)m->Vp, c.pad_id};
        static int fuse_dh = -1;     // the head's input gradient inside the same launch (KZV_HEAD_DGRAD=0: the separate GEMM)
        if (fuse_dh < 0) fuse_dh = kzv_env_int("KZV_HEAD_DGRAD", 1);
        m->dhln_fused = m->train && fuse_dh && m->word.h.ldt % 8 == 0;
        if (m->dhln_fused) { hc.wpt = m->dec_pack.as<bf16_t>() + pk.head_t(); hc.dh = m->dhln; }
        hc.label_smoothing = ls_eps; hc.class_weights = cls_w; hc.focal_gamma = focal;
        KZV_TRY(kzv_head_ce(hc, s));
    } else {
        m->dhln_fused = false;
        KZV_TRY(lin_fwd(m, m->word, m->hd_ln, Hd, Md, m->logits, m->Vp, KZV_EPI_F32, s, {.n = m->Vp}));
        KZV_TRY(kzv_ce_fwd_bwd(m->logits, m->Vp, labels, m->L, B, T, m->V, c.pad_id, norm, m->loss_acc, m->train ? m->dlogits : nullptr, ls_eps, s, cls_w, focal));
    }
    if (d_loss && hipMemcpyAsync(d_loss, m->loss_acc, sizeof(float), hipMemcpyDeviceToDevice, s) != hipSuccess)
        return kzv_fail(KZV_E_HIP, "forward: loss copy");
    if (d_logits && logits_pos < 0) {
        if (T != m->T) return kzv_fail(KZV_E_STATE, "forward_loss: full logits need the full decoder length (kzv_set_active_length(m, L-1))");
        KZV_TRY(kzv_copy_logits(m->logits, m->Vp, d_logits, Md, m->V, s));
    }
    if (d_logits && logits_pos >= 0)   // one position of every sample: rows b*T + pos
        KZV_TRY(kzv_copy_logits(m->logits + (int64_t)logits_pos * m->Vp, (int64_t)T * m->Vp, d_logits, B, m->V, s));
    return KZV_OK;
}

// ============================================================================================== backward
int backward_decoder(kzv_model* m, hipStream_t s) {
    const kzv_config& c = m->c;
    const int B = m->B, T = m->Ta, Hd = m->Hd, Fd = m->Fd, He = m->He;
    const int Mp = B * m->npa, Md = B * T, Me = B * m->Sa;
    float* P = m->P; float* G = m->G;
    const int CK = m->Ld * 2 * Hd;
    m->wbatch.clear();
    // the decoder's input-gradient GEMMs on the row-panel kernel (decoder_chain_bwd.hip kzv_dec_lin) where the forward's fragment-ordered
    // packs exist (the reference decoder's geometry, chains on): transposed packs, same layout as the forward's
    static int dgrad_rows = -1;          // dev A/B: KZV_DEC_DGRAD=0 keeps the 128 x 128 kernel for these
    if (dgrad_rows < 0) dgrad_rows = kzv_env_int("KZV_DEC_DGRAD", 1);
    const bool rows_dgrad = dgrad_rows && dec_chain_mode() && dec_packable(m) && m->dec_pack_ok && !m->use_side;
    // measured (profiles/r04): the 256 x 256 products take 7.8 / 12.6 us there against ~16 us on the 128 x 128 kernel; the 768-wide ones
    // (fc2's DGELU output, the K = 768 reductions of fc1 / qkv) are SLOWER on it (35 / 21 us against 22 / 16 - 22): they keep gemm_nt
    static int wide_rows = -1;
    if (wide_rows < 0) wide_rows = kzv_env_int("KZV_DEC_DGRAD_WIDE", 0);
    const bool rows_wide = rows_dgrad && wide_rows;
    const DecPack& pk = m->pk;
    auto tp = [&](int layer, DecPack::Which w) { return (const bf16_t*)(m->dec_pack.as<bf16_t>() + pk.tr(layer, w)); };
    const float hp = dp(m, c.dec_hidden_dropout);
    // ---- CE -> LM head ------------------------------------------------------------------------------
    KZV_TRY(lin_wgrad_batch(m, m->word, CLS_MISC, s, m->dlogits, m->Vp, m->hd_ln, Hd, Md, {.n = m->Vp}));
    if (!m->dhln_fused) KZV_TRY(lin_dgrad(m, m->word, m->dlogits, m->Vp, Md, m->dhln, Hd, KZV_EPI_BF16, s, {.n = m->Vp}));
    KZV_TRY(ln_bwd(m, m->dhln, 0, m->hd_gelu, m->hd_st, m->hln_w, m->hln_b, m->dsum_d, 0, Md, Hd, s));
    KZV_TRY(kzv_cast_drop_colsum(m->dsum_d, m->dy_d, G + m->hd.b, Md, Hd, 0.f, 0, s, m->hd_pre));
    const bf16_t* x_last_h = m->Ld ? m->da[m->Ld - 1].x3h : m->xd0h;
    KZV_TRY(lin_wgrad_batch(m, m->hd, CLS_DY, s, m->dy_d, Hd, x_last_h, Hd, Md, {.bias = false}));
    // the three row-local segments of a layer's backward, one launch each (decoder_chain_bwd.hip dec_bwd_seg_kernel): the head dense's input
    // gradient becomes the first GEMM of the top layer's first segment
    const bool segs = rows_dgrad && dec_chain_mode() >= 2 && m->Ld > 0;
    if (!segs) {
        if (rows_dgrad) KZV_TRY(kzv_dec_lin(m->dy_d, m->dec_pack.as<bf16_t>() + pk.head_dense_t(), m->dx_d, nullptr, nullptr, Md, Hd, Hd, 1, s));
        else KZV_TRY(lin_dgrad(m, m->hd, m->dy_d, Hd, Md, m->dx_d, Hd, KZV_EPI_F32, s));
    }
    KZV_TRY(wgrad_flush(m, s));          // LM head (tied word embedding) + head dense: before dy_d is rewritten
    // ---- decoder layers, last to first -----------------------------------------------------------------
    for (int i = m->Ld - 1; i >= 0; --i) {
        DecAct& a = m->da[i];
        const DecLayerP& d = m->dp[i];
        const uint32_t site = SITE_DEC_L + 8 * i;
        const bf16_t* xh = i ? m->da[i - 1].x3h : m->xd0h;
        const AttnSite sa = dec_self(m, i), ca = dec_cross(m, i);
        bf16_t* dckv = cross_dkv(m, i);
        if (segs) {
            const bool top = i == m->Ld - 1;
            // every "dY" of this layer goes to the layer's own buffers: the 6 x Ld weight gradients are ONE grouped launch behind the loop
            // (36 problems, 288 tiles of 128 x 128 over all tokens instead of six part-filled grids of ten token splits and their atomics)
            // [head dense | the layer above's qkv] -> LN3 -> fc2 (gelu')
            KZV_TRY(kzv_dec_bwd_seg(KzvDecBwdSeg{top ? m->dy_d : m->da[i + 1].g_dqkv, top ? Hd : 3 * Hd,
                                                 top ? m->dec_pack.as<bf16_t>() + pk.head_dense_t() : tp(i + 1, DecPack::QKV), top ? nullptr : m->dsum_d,
                                                 a.s3, a.st3, P + d.ln3w, G + d.ln3w, G + d.ln3b, m->dsum_d, a.g_dy, hp, key(m, site + 4),
                                                 tp(i, DecPack::FC2), a.pre, a.g_dbig, Md}, s));
            KZV_TRY(lin_wgrad_batch(m, d.fc2, CLS_DY, s, a.g_dy, Hd, a.act, Fd, Md));
            KZV_TRY(lin_wgrad_batch(m, d.fc1, CLS_DBIG, s, a.g_dbig, Fd, a.x2h, Hd, Md));
            // fc1 -> LN2 -> cross-attention output projection
            KZV_TRY(kzv_dec_bwd_seg(KzvDecBwdSeg{a.g_dbig, Fd, tp(i, DecPack::FC1), m->dsum_d, a.s2, a.st2, P + d.ln2w, G + d.ln2w, G + d.ln2b, m->dsum_d, a.g_dy2,
                                                 hp, key(m, site + 3), tp(i, DecPack::CO), nullptr, m->dctx_d, Md}, s));
            KZV_TRY(lin_wgrad_batch(m, d.co, CLS_DY, s, a.g_dy2, Hd, a.cctx, Hd, Md));
            KZV_TRY(attn_bwd(m, ca, m->dctx_d, a.g_dq, dckv, dckv + Hd, s));
            KZV_TRY(lin_wgrad_batch(m, d.cq, CLS_MISC, s, a.g_dq, Hd, a.x1h, Hd, Md));
            // cross-attention query -> LN1 -> self-attention output projection
            KZV_TRY(kzv_dec_bwd_seg(KzvDecBwdSeg{a.g_dq, Hd, tp(i, DecPack::CQ), m->dsum_d, a.s1, a.st1, P + d.ln1w, G + d.ln1w, G + d.ln1b, m->dsum_d, a.g_dy3,
                                                 hp, key(m, site + 1), tp(i, DecPack::O), nullptr, m->dctx_d, Md}, s));
            KZV_TRY(lin_wgrad_batch(m, d.o, CLS_DY, s, a.g_dy3, Hd, a.ctx, Hd, Md));
            KZV_TRY(attn_bwd(m, sa, m->dctx_d, a.g_dqkv, a.g_dqkv + Hd, a.g_dqkv + 2 * Hd, s));
            KZV_TRY(lin_wgrad_batch(m, d.qkv, CLS_DQKV, s, a.g_dqkv, 3 * Hd, xh, Hd, Md));
            if (i == 0) {    // the bottom layer's qkv feeds the embedding LayerNorm: its own launch (a lower layer's first segment takes it otherwise)
                KZV_TRY(lin_dgrad(m, d.qkv, a.g_dqkv, 3 * Hd, Md, m->dx_d, Hd, KZV_EPI_RESID, s, {.resid = m->dsum_d}));
                KZV_TRY(wgrad_flush(m, s));      // all 6 x Ld weight gradients of the decoder layers
            }
            continue;
        }
        // FFN block: x3 = LN(s3), s3 = x2 + drop(fc2(gelu(fc1(x2))))
        KZV_TRY(wait_cls(m, CLS_DY, s));
        KZV_TRY(ln_bwd(m, m->dx_d, 1, a.s3, a.st3, d.ln3w, d.ln3b, m->dsum_d, 0, Md, Hd, s, {.out16 = m->dy_d, .out_drop_p = hp, .out_drop_key = key(m, site + 4)}));
        KZV_TRY(lin_wgrad_batch(m, d.fc2, CLS_DY, s, m->dy_d, Hd, a.act, Fd, Md));
        KZV_TRY(wait_cls(m, CLS_DBIG, s));
        if (rows_wide) KZV_TRY(kzv_dec_lin(m->dy_d, tp(i, DecPack::FC2), m->dbig_d, nullptr, a.pre, Md, Fd, Hd, 2, s));
        else KZV_TRY(lin_dgrad(m, d.fc2, m->dy_d, Hd, Md, m->dbig_d, Fd, KZV_EPI_DGELU, s, {.aux = a.pre, .ldaux = Fd}));
        KZV_TRY(lin_wgrad_batch(m, d.fc1, CLS_DBIG, s, m->dbig_d, Fd, a.x2h, Hd, Md));
        if (rows_wide) KZV_TRY(kzv_dec_lin(m->dbig_d, tp(i, DecPack::FC1), m->dx_d, m->dsum_d, nullptr, Md, Hd, Fd, 1, s));
        else KZV_TRY(lin_dgrad(m, d.fc1, m->dbig_d, Fd, Md, m->dx_d, Hd, KZV_EPI_RESID, s, {.resid = m->dsum_d}));
        // cross-attention block: x2 = LN(s2), s2 = x1 + drop(o(CA(q(x1), kv(enc))))
        KZV_TRY(wait_cls(m, CLS_DY, s));
        bf16_t* dy2 = m->use_side ? m->dy_d : m->dy_d2;      // grouped launch: the three dy of a layer stay alive until its end
        bf16_t* dy3 = m->use_side ? m->dy_d : m->dy_d3;
        KZV_TRY(ln_bwd(m, m->dx_d, 1, a.s2, a.st2, d.ln2w, d.ln2b, m->dsum_d, 0, Md, Hd, s, {.out16 = dy2, .out_drop_p = hp, .out_drop_key = key(m, site + 3)}));
        KZV_TRY(lin_wgrad_batch(m, d.co, CLS_DY, s, dy2, Hd, a.cctx, Hd, Md));
        KZV_TRY(wait_cls(m, CLS_MISC, s));   // dq_d (and, first layer, dlogits' reader) before the cross-attention backward rewrites dq_d
        if (rows_dgrad) KZV_TRY(kzv_dec_lin(dy2, tp(i, DecPack::CO), m->dctx_d, nullptr, nullptr, Md, Hd, Hd, 0, s));
        else KZV_TRY(lin_dgrad(m, d.co, dy2, Hd, Md, m->dctx_d, Hd, KZV_EPI_BF16, s));
        KZV_TRY(attn_bwd(m, ca, m->dctx_d, m->dq_d, dckv, dckv + Hd, s));
        KZV_TRY(lin_wgrad_batch(m, d.cq, CLS_MISC, s, m->dq_d, Hd, a.x1h, Hd, Md));
        if (rows_dgrad) KZV_TRY(kzv_dec_lin(m->dq_d, tp(i, DecPack::CQ), m->dx_d, m->dsum_d, nullptr, Md, Hd, Hd, 1, s));
        else KZV_TRY(lin_dgrad(m, d.cq, m->dq_d, Hd, Md, m->dx_d, Hd, KZV_EPI_RESID, s, {.resid = m->dsum_d}));
        // self-attention block: x1 = LN(s1), s1 = x + drop(o(SA(qkv(x))))
        KZV_TRY(wait_cls(m, CLS_DY, s));
        KZV_TRY(ln_bwd(m, m->dx_d, 1, a.s1, a.st1, d.ln1w, d.ln1b, m->dsum_d, 0, Md, Hd, s, {.out16 = dy3, .out_drop_p = hp, .out_drop_key = key(m, site + 1)}));
        KZV_TRY(lin_wgrad_batch(m, d.o, CLS_DY, s, dy3, Hd, a.ctx, Hd, Md));
        KZV_TRY(wait_cls(m, CLS_DQKV, s));
        if (rows_dgrad) KZV_TRY(kzv_dec_lin(dy3, tp(i, DecPack::O), m->dctx_d, nullptr, nullptr, Md, Hd, Hd, 0, s));
        else KZV_TRY(lin_dgrad(m, d.o, dy3, Hd, Md, m->dctx_d, Hd, KZV_EPI_BF16, s));
        KZV_TRY(attn_bwd(m, sa, m->dctx_d, m->dqkv_d, m->dqkv_d + Hd, m->dqkv_d + 2 * Hd, s));
        KZV_TRY(lin_wgrad_batch(m, d.qkv, CLS_DQKV, s, m->dqkv_d, 3 * Hd, xh, Hd, Md));
        if (rows_wide) KZV_TRY(kzv_dec_lin(m->dqkv_d, tp(i, DecPack::QKV), m->dx_d, m->dsum_d, nullptr, Md, Hd, 3 * Hd, 1, s));
        else KZV_TRY(lin_dgrad(m, d.qkv, m->dqkv_d, 3 * Hd, Md, m->dx_d, Hd, KZV_EPI_RESID, s, {.resid = m->dsum_d}));
        KZV_TRY(wgrad_flush(m, s));      // the six weight gradients of this layer in one grid
    }
    // ---- decoder embeddings: x0 = drop(LN(word + type + pos)) ---------------------------------------------
    KZV_TRY(ln_bwd(m, m->dx_d, 1, m->emb_sum, m->emb_st, m->eln_w, m->eln_b, m->dsum_d, 0, Md, Hd, s, {.drop_p = hp, .drop_key = key(m, SITE_DEC_EMB)}));
    KZV_TRY(kzv_embed_scatter_bwd(m->dsum_d, m->labels, m->L, m->posids, G + m->word.w, G + m->dtype, G + m->dpos, B, T, Hd, c.pad_id, s));
    // ---- cross K/V projection of all layers, encoder_decoder_proj, final encoder LN ---------------------------
    KZV_TRY(lin_wgrad_batch(m, m->ckv, CLS_MISC, s, m->dckv, CK, m->proj_out, Hd, Mp));
    KZV_TRY(lin_dgrad(m, m->ckv, m->dckv, CK, Mp, m->denc, Hd, KZV_EPI_BF16, s));
    if (m->has_proj) {
        KZV_TRY(lin_wgrad_batch(m, m->proj, CLS_DQKV, s, m->denc, Hd, m->enc_out, He, Mp));
        KZV_TRY(lin_dgrad(m, m->proj, m->denc, Hd, Mp, m->denc_out, He, KZV_EPI_BF16, s));
    }
    KZV_TRY(wgrad_flush(m, s));          // cross-attention K/V of all layers + encoder_decoder_proj
    // also emits the masked bf16 copy the top ViT layer's fc2 backward starts from
    KZV_TRY(wait_cls(m, CLS_DY, s));
    const KzvLnBwdF8 f8top{m->dy8, m->dy8_scale, m->dy8_rq, m->dy8_rqinv, m->f8_wnorm ? m->f8_wnorm + (m->Le - 1) : nullptr};
    KZV_TRY(ln_bwd(m, m->denc_out, 0, m->x_last, m->stf, m->lnf_w, m->lnf_b, m->dx_e, 0, Me, He, s,
                   {.seq = m->Sa, .drop_first = 1, .out16 = m->Le ? m->dy_e : nullptr, .out_drop_p = dp(m, c.enc_hidden_dropout),
                    .out_drop_key = key(m, SITE_ENC_L + 4 * (m->Le - 1) + 2), .f8 = (m->fp8 >= 2 && m->Le && !m->use_side) ? &f8top : nullptr}));
    return KZV_OK;
}

int backward_enc_layer(kzv_model* m, int i, hipStream_t s) {
    const kzv_config& c = m->c;
    const int He = m->He, Fe = m->Fe, Me = m->B * m->Sa;
    EncAct& a = m->ea[i];
    const EncLayerP& e = m->ep[i];
    const AttnSite sa = enc_self(m, i, m->B);
    const float hp = dp(m, c.enc_hidden_dropout);
    // the masked bf16 copy of dx_e a LayerNorm backward leaves for the Linear below it: this layer's output projection (LN2) and the fc2 of
    // the layer below (LN1; layer 0 hands fp32 dx_e to the embedding backward)
    const uint32_t key_o = key(m, SITE_ENC_L + 4 * i + 1), key_fc2_below = key(m, SITE_ENC_L + 4 * (i - 1) + 2);
    // the layer's four weight-gradient GEMMs fold their partial tiles in one launch at the end of the layer (one stream only)
    std::optional<KzvTnFoldScope> tn_folds;
    if (!m->use_side) tn_folds.emplace(s);
    if (m->side_mode == 2) {
        // Overlap mode 2: the four weight-gradient GEMMs (MFMA-bound, 710 us per layer) run on the side stream ONLY while
        // the caller's stream runs an HBM- or issue-bound kernel (LayerNorm backward x2, attention backward: 344 us per
        // layer); every input-gradient GEMM first joins the side stream, so the gemm_nt kernels never share the machine
        // (their per-launch times stay what they are alone) and nothing MFMA-bound competes with anything MFMA-bound.
        struct SideOk { kzv_model* m; ~SideOk() { m->side_ok = false; } } side_guard{m};
        m->side_ok = true;
        KZV_TRY(join_side(m, s));
        KZV_TRY(lin_dgrad(m, e.fc2, m->dy_e, He, Me, m->dbig_e, Fe, KZV_EPI_DGELU, s, {.aux = a.pre, .ldaux = Fe}));
        KZV_TRY(lin_dgrad(m, e.fc1, m->dbig_e, Fe, Me, m->dh_e, He, KZV_EPI_BF16, s));
        KZV_TRY(lin_wgrad(m, e.fc2, CLS_DY, s, m->dy_e, He, a.act, Fe, Me));
        KZV_TRY(ln_bwd(m, m->dh_e, 0, a.x_mid, a.st2, e.ln2w, e.ln2b, m->dx_e, 1, Me, He, s, {.out16 = m->dy_e2, .out_drop_p = hp, .out_drop_key = key_o}));
        KZV_TRY(join_side(m, s));
        KZV_TRY(lin_dgrad(m, e.o, m->dy_e2, He, Me, m->dctx_e, He, KZV_EPI_BF16, s));
        KZV_TRY(lin_wgrad(m, e.o, CLS_DY, s, m->dy_e2, He, a.ctx, He, Me));
        KZV_TRY(lin_wgrad(m, e.fc1, CLS_DBIG, s, m->dbig_e, Fe, a.ln2, He, Me));
        KZV_TRY(attn_bwd(m, sa, m->dctx_e, m->dqkv_e, m->dqkv_e + He, m->dqkv_e + 2 * He, s));
        KZV_TRY(join_side(m, s));
        KZV_TRY(lin_dgrad(m, e.qkv, m->dqkv_e, 3 * He, Me, m->dh_e, He, KZV_EPI_BF16, s));
        KZV_TRY(lin_wgrad(m, e.qkv, CLS_DQKV, s, m->dqkv_e, 3 * He, a.ln1, He, Me));
        KZV_TRY(ln_bwd(m, m->dh_e, 0, a.x_in, a.st1, e.ln1w, e.ln1b, m->dx_e, 1, Me, He, s,
                       {.out16 = i > 0 ? m->dy_e : nullptr, .out_drop_p = hp, .out_drop_key = key_fc2_below}));
        return tn_folds ? tn_folds->close() : KZV_OK;
    }
    // x_out = x_mid + drop(fc2(gelu(fc1(LN2(x_mid)))))
    // on entry dy_e = dropout-masked bf16 copy of dx_e for this layer's fc2 site (written by the LN backward above it)
    const bool f8g = m->fp8 >= 2 && !m->use_side;       // e4m3 input-gradient GEMMs of the MLP (the weight gradients keep reading bf16)
    if (f8g) {
        KZV_TRY(lin_wgrad(m, e.fc2, CLS_DY, s, m->dy_e, He, a.act, Fe, Me));
        KZV_TRY(wait_cls(m, CLS_DBIG, s));
        KZV_TRY(lin_dgrad(m, e.fc2, nullptr, 0, Me, m->dbig_e, Fe, KZV_EPI_DGELU, s,
                          {.aux = a.pre, .ldaux = Fe, .a8 = m->dy8, .a8_scale = m->dy8_scale, .c8 = m->dbig8, .c8_rowq = m->dy8_rq}));
        KZV_TRY(lin_wgrad(m, e.fc1, CLS_DBIG, s, m->dbig_e, Fe, a.ln2, He, Me));
        KZV_TRY(lin_dgrad(m, e.fc1, nullptr, 0, Me, m->dh_e, He, KZV_EPI_BF16, s, {.a8 = m->dbig8, .a8_scale = m->dy8_rqinv}));
    } else {
        // each Linear's input gradient and weight gradient read the same dY: one launch per pair where the 256x256 kernels take both
        KZV_TRY(wait_cls(m, CLS_DBIG, s));
        KZV_TRY(dgrad_wgrad(m, e.fc2, CLS_DY, s, m->dy_e, He, Me, m->dbig_e, Fe, KZV_EPI_DGELU, a.act, Fe, {.aux = a.pre, .ldaux = Fe}));
        KZV_TRY(dgrad_wgrad(m, e.fc1, CLS_DBIG, s, m->dbig_e, Fe, Me, m->dh_e, He, KZV_EPI_BF16, a.ln2, He));
    }
    KZV_TRY(wait_cls(m, CLS_DY, s));      // dy_e is rewritten below
    KZV_TRY(ln_bwd(m, m->dh_e, 0, a.x_mid, a.st2, e.ln2w, e.ln2b, m->dx_e, 1, Me, He, s, {.out16 = m->dy_e, .out_drop_p = hp, .out_drop_key = key_o}));
    // x_mid = x_in + drop(o(attn(qkv(LN1(x_in)))))
    KZV_TRY(dgrad_wgrad(m, e.o, CLS_DY, s, m->dy_e, He, Me, m->dctx_e, He, KZV_EPI_BF16, a.ctx, He));
    KZV_TRY(wait_cls(m, CLS_DQKV, s));    // dqkv_e is rewritten below
    KZV_TRY(attn_bwd(m, sa, m->dctx_e, m->dqkv_e, m->dqkv_e + He, m->dqkv_e + 2 * He, s));
    KZV_TRY(dgrad_wgrad(m, e.qkv, CLS_DQKV, s, m->dqkv_e, 3 * He, Me, m->dh_e, He, KZV_EPI_BF16, a.ln1, He));
    // ... and the masked copy for the fc2 site of the layer below
    KZV_TRY(wait_cls(m, CLS_DY, s));
    const KzvLnBwdF8 f8n{m->dy8, m->dy8_scale, m->dy8_rq, m->dy8_rqinv, (m->f8_wnorm && i > 0) ? m->f8_wnorm + (i - 1) : nullptr};
    KZV_TRY(ln_bwd(m, m->dh_e, 0, a.x_in, a.st1, e.ln1w, e.ln1b, m->dx_e, 1, Me, He, s,
                   {.out16 = i > 0 ? m->dy_e : nullptr, .out_drop_p = hp, .out_drop_key = key_fc2_below, .f8 = (f8g && i > 0) ? &f8n : nullptr}));
    return tn_folds ? tn_folds->close() : KZV_OK;
}

int backward_embed(kzv_model* m, hipStream_t s) {
    const kzv_config& c = m->c;
    const int He = m->He, Mp = m->B * m->npa;
    float* G = m->G;
    KZV_TRY(kzv_embed_assemble_bwd(m->dx_e, m->dpatch, G + m->cls, G + m->pos, G + m->patch.b, m->B, m->npa, He,
                                   dp(m, c.enc_hidden_dropout), key(m, SITE_ENC_EMB), s, m->img_w / c.patch_w, c.image_w / c.patch_w));
    KZV_TRY(lin_wgrad(m, m->patch, CLS_MISC, s, m->dpatch, He, m->patches, m->PD, Mp, {.bias = false}));
    return KZV_OK;
}

// ================================================================================================== C ABI
extern "C" int kzv_forward_loss(kzv_model* m, const float* d_pixel_values, const int64_t* d_labels, float* d_loss,
                                float* d_logits, int train, uint64_t seed, void* stream) {
    if (!m || !m->bound) return kzv_fail(KZV_E_STATE, "forward_loss: model not bound");
    if (!d_pixel_values || !d_labels) return kzv_fail(KZV_E_ARG, "forward_loss: null input");
    m->train = train != 0; m->seed = seed;
    const int rc = forward(m, d_pixel_values, d_labels, d_loss, d_logits, (hipStream_t)stream);
    m->have_fwd = rc == KZV_OK && m->train;
    m->have_dec = rc == KZV_OK;
    return rc;
}

extern "C" int kzv_check_positions(kzv_model* m, void* stream) {
    if (!m || !m->bound) return kzv_fail(KZV_E_STATE, "check_positions: model not bound");
    int flag = 0;
    if (hipMemcpyAsync(&flag, m->err, sizeof(int), hipMemcpyDeviceToHost, (hipStream_t)stream) != hipSuccess ||
        hipStreamSynchronize((hipStream_t)stream) != hipSuccess)
        return kzv_fail(KZV_E_HIP, "check_positions: copy");
    if (flag) return kzv_fail(KZV_E_ARG, "labels too long: a position id reached max_position_embeddings = %d (index out of range in the reference)", m->c.max_pos);
    return KZV_OK;
}

extern "C" int kzv_encode_images(kzv_model* m, const float* d_pixel_values, int n_images, void* stream) {
    if (!m || !m->bound) return kzv_fail(KZV_E_STATE, "encode_images: model not bound");
    if (!d_pixel_values || n_images < 1 || n_images > m->B || m->B % n_images)
        return kzv_fail(KZV_E_ARG, "encode_images: 1 <= n_images <= bound batch %d, which must be a multiple of it", m->B);
    m->train = false; m->seed = 0; m->have_fwd = false; m->have_dec = false;
    return forward(m, d_pixel_values, nullptr, nullptr, nullptr, (hipStream_t)stream, true, -1, n_images, false);
}

extern "C" int kzv_decode_logits(kzv_model* m, const int64_t* d_labels, int pos, float* d_logits, void* stream) {
    if (!m || !m->bound) return kzv_fail(KZV_E_STATE, "decode_logits: model not bound");
    if (!m->have_enc) return kzv_fail(KZV_E_STATE, "decode_logits: call kzv_forward_loss on the images first");
    if (!d_labels || !d_logits || pos < 0 || pos >= m->Ta) return kzv_fail(KZV_E_ARG, "decode_logits: position outside the active decoder length");
    m->train = false;
    m->have_fwd = false; m->have_dec = false;     // decoder activations are overwritten: no backward after this
    return forward(m, nullptr, d_labels, nullptr, d_logits, (hipStream_t)stream, false, pos);
}

// ---- read-backs of the last forward's decoder activations (have_dec) -----------------------------------------------------------------
extern "C" int kzv_cross_attention(kzv_model* m, int layer, float* d_map, int64_t ld_map, float* d_pos, int32_t* d_peak, void* stream) {
    if (!m || !m->bound) return kzv_fail(KZV_E_STATE, "cross_attention: model not bound");
    if (!m->have_dec) return kzv_fail(KZV_E_STATE, "cross_attention: call kzv_forward_loss first (its decoder activations are gone or were never computed)");
    if (layer < -1 || layer >= m->Ld) return kzv_fail(KZV_E_ARG, "cross_attention: layer must be in -1..%d", m->Ld - 1);
    const AttnSite t = dec_cross(m, layer < 0 ? m->Ld - 1 : layer);
    kzv_attn_probs_args a;
    memset(&a, 0, sizeof(a));
    a.Q = t.Q; a.K = t.K; a.ldq = t.ldq; a.ldk = t.ldkv; a.LSE = t.LSE;
    a.map = d_map; a.ld_map = ld_map; a.pos = d_pos; a.peak = d_peak;
    a.B = t.batch; a.heads = t.heads; a.Sq = t.Sq; a.Sk = t.Sk; a.grid_w = m->img_w / m->c.patch_w; a.head_dim = t.head_dim; a.mode = t.mode;
    return kzv_attn_probs(&a, stream);
}

extern "C" int kzv_score_tokens(kzv_model* m, float* d_logprob, int64_t* d_top1, float* d_top1_logprob, void* stream) {
    if (!m || !m->bound) return kzv_fail(KZV_E_STATE, "score_tokens: model not bound");
    if (!m->have_dec) return kzv_fail(KZV_E_STATE, "score_tokens: call kzv_forward_loss first (its decoder activations are gone or were never computed)");
    hipStream_t s = (hipStream_t)stream;
    // the vocabulary GEMM of forward()'s non-fused branch, from the saved LM-head input into the logits region (the fused head + CE path
    // never wrote it; the backward reads dlogits and hd_ln, not logits)
    KZV_TRY(lin_fwd(m, m->word, m->hd_ln, m->Hd, m->B * m->Ta, m->logits, m->Vp, KZV_EPI_F32, s, {.n = m->Vp}));
    return kzv_token_scores(m->logits, m->Vp, m->labels, m->L, m->B, m->Ta, m->V, m->c.pad_id, d_logprob, d_top1, d_top1_logprob, stream);
}

extern "C" int kzv_score_tokens_topk(kzv_model* m, int k, int32_t* d_ids, float* d_logprob, void* stream) {
    if (!m || !m->bound) return kzv_fail(KZV_E_STATE, "score_tokens_topk: model not bound");
    if (!m->have_dec) return kzv_fail(KZV_E_STATE, "score_tokens_topk: call kzv_forward_loss first (its decoder activations are gone or were never computed)");
    if (k < 1 || k > 8 || !d_ids || !d_logprob) return kzv_fail(KZV_E_ARG, "score_tokens_topk: k in 1..8 and two result arrays [B, t_active, k]");
    // kzv_score_tokens' vocabulary GEMM, then the k best columns of every packed row
    KZV_TRY(lin_fwd(m, m->word, m->hd_ln, m->Hd, m->B * m->Ta, m->logits, m->Vp, KZV_EPI_F32, (hipStream_t)stream, {.n = m->Vp}));
    return kzv_token_topk(m->logits, m->Vp, (int64_t)m->B * m->Ta, m->V, k, d_ids, d_logprob, stream);
}

extern "C" int kzv_backward_segments(const kzv_model* m) { return m ? m->Le + 2 : 0; }

extern "C" int kzv_backward_segment_range(const kzv_model* m, int seg, int64_t* lo, int64_t* hi) {
    if (!m || seg < 0 || seg >= m->Le + 2) return kzv_fail(KZV_E_ARG, "segment_range: bad segment");
    int64_t a, b;
    if (seg == 0) { a = m->lnf_w; b = m->total; }                                   // decoder + proj + final LN
    else if (seg <= m->Le) {                                                         // encoder layer Le - seg
        const int i = m->Le - seg;
        a = m->ep[i].ln1w; b = i + 1 < m->Le ? m->ep[i + 1].ln1w : m->lnf_w;
    } else { a = 0; b = m->Le ? m->ep[0].ln1w : m->lnf_w; }                            // patch / cls / pos
    if (lo) *lo = a;
    if (hi) *hi = b;
    return KZV_OK;
}

extern "C" int kzv_backward_segment(kzv_model* m, int seg, void* stream) {
    if (!m || !m->bound || !m->G) return kzv_fail(KZV_E_STATE, "backward: no gradient buffer bound");
    if (!m->have_fwd) return kzv_fail(KZV_E_STATE, "backward: call kzv_forward_loss(train=1) first");
    if (seg < 0 || seg >= m->Le + 2) return kzv_fail(KZV_E_ARG, "backward: bad segment");
    // frozen bottom of the encoder: the segments below the cut launch nothing, the last one above it does the final join
    const int last_seg = m->frozen_enc > 0 ? m->Le - m->frozen_enc : m->Le + 1;
    if (seg > last_seg) return KZV_OK;
    hipStream_t s = (hipStream_t)stream;
    int rc;
    {
        KzvLnDeferScope ln_folds(s);             // the segment's LayerNorm gamma / beta folds: one launch when the scope closes (under
        if (seg == 0) rc = backward_decoder(m, s);              // kzv_backward: when ITS scope closes, once per backward pass)
        else if (seg <= m->Le) rc = backward_enc_layer(m, m->Le - seg, s);
        else rc = backward_embed(m, s);
        const int folds = ln_folds.close();
        if (rc == KZV_OK) rc = folds;
    }
    if (rc != KZV_OK) return rc;
    // contract: in `stream` order, this segment's gradient range is final -> the side stream must be joined
    // (kzv_backward, which has no consumer between segments, joins once at the end instead)
    if (m->join_each_segment || seg == last_seg) return join_side(m, s);
    return KZV_OK;
}

extern "C" int kzv_backward(kzv_model* m, void* stream) {
    if (!m) return kzv_fail(KZV_E_STATE, "backward: null model");
    const int n = kzv_backward_segments(m);
    m->join_each_segment = false;
    int rc = KZV_OK;
    {
        KzvLnDeferScope ln_folds((hipStream_t)stream);
        for (int sgm = 0; sgm < n && rc == KZV_OK; ++sgm) rc = kzv_backward_segment(m, sgm, stream);
        const int folds = ln_folds.close();
        if (rc == KZV_OK) rc = folds;
    }
    m->join_each_segment = true;
    if (rc != KZV_OK) (void)join_side(m, (hipStream_t)stream);
    return rc;
}
