// The model handle and what its four units share (model.cpp: table, plan, bind; model_train.cpp: forward / backward schedules;
// model_decode.cpp: lockstep generation steps; model_stream.cpp: slot-refill decoding): the handle itself, one descriptor per Linear (Lin), the fragment-pack layout (DecPack),
// and the call helpers that take their shapes, weight copies and gradient destinations from a Lin instead of positional arguments.
// Nothing declared here is part of the library's dynamic symbol table.
#pragma once
#include "kzv_host.h"
#include "kzv_kernels.h"
#include "../../include/kzv.h"
#include "gemm_nt.h"
#include "gemm_tn.h"
#include "attention_common.h"
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#pragma GCC visibility push(hidden)
#pragma clang diagnostic ignored "-Wc++20-designator"      // the units initialise the option aggregates below by field name

#define KZV_TRY(expr) do { int rc__ = (expr); if (rc__ != KZV_OK) return rc__; } while (0)

struct PEntry { std::string name; int64_t off, rows, cols; };

inline int64_t align_up(int64_t n, int64_t a) { return (n + a - 1) / a * a; }

struct W16 { bf16_t* w; bf16_t* wt; int64_t ldt; };   // bf16 copy [N,K] and transposed copy [K, ldt]
struct W8 { unsigned char* w; float* scale; };         // fp8 path: e4m3 copy [N,K] quantised per output row, scale [N]
// One Linear: fp32 offsets of weight [N,K] and bias [N] into P and G, its bf16 copies, and (fp8 path, some encoder linears) the e4m3
// copy q and the e4m3 copy qt of the transposed weight
struct Lin { int64_t w = 0, b = 0; int N = 0, K = 0; W16 h{}; W8 q{}, qt{}; };

struct EncLayerP { int64_t ln1w, ln1b, ln2w, ln2b; Lin qkv, o, fc1, fc2; };
struct DecLayerP { int64_t ln1w, ln1b, ln2w, ln2b, ln3w, ln3b; Lin qkv, o, cq, co, fc1, fc2; };

struct EncAct {
    float *x_in, *x_mid, *st1, *st2, *lse;
    bf16_t *ln1, *qkv, *ctx, *ln2, *pre, *act;
};
struct DecAct {
    float *s1, *x1, *s2, *x2, *s3, *x3, *st1, *st2, *st3, *lse_sa, *lse_ca;
    bf16_t *qkv, *ctx, *x1h, *cq, *cctx, *x2h, *pre, *act, *x3h;
    // backward (segment path): this layer's six "dY" operands stay alive until ONE grouped weight-gradient launch behind the last layer
    bf16_t *g_dy = nullptr, *g_dbig = nullptr, *g_dy2 = nullptr, *g_dq = nullptr, *g_dy3 = nullptr, *g_dqkv = nullptr;
};

// The decoder's bf16 weights in MFMA fragment order (decode_fused.hip, the dec_rows.h family; packed by frag_pack.hip), element offsets into kzv_model::dec_pack:
//   [layer 0..Ld-1: qkv | o | cq | co | fc1 | fc2] [head dense] [tied LM head, vq rows] then the same again TRANSPOSED ([in, out]
//   row-major, the B operands of the input-gradient GEMMs).  vq = the vocabulary in 256-row chunks (zeros beyond it).
struct DecPack {
    enum Which { QKV, O, CQ, CO, FC1, FC2 };
    int64_t HH = 0, FH = 0, per = 0, half = 0; int Ld = 0, vq = 0;
    DecPack() = default;
    DecPack(int Hd, int Fd, int layers, int V) : HH((int64_t)Hd * Hd), FH((int64_t)Fd * Hd), per(6 * HH + 2 * FH), Ld(layers), vq((V + 255) / 256 * 256) {
        half = per * Ld + HH + (int64_t)vq * Hd;
    }
    int64_t in_layer(Which w) const { return w == QKV ? 0 : w <= CO ? (2 + (int)w) * HH : w == FC1 ? 6 * HH : 6 * HH + FH; }
    int64_t fwd(int layer, Which w) const { return per * layer + in_layer(w); }
    int64_t head_dense() const { return per * Ld; }
    int64_t head() const { return per * Ld + HH; }
    int64_t tr(int layer, Which w) const { return half + fwd(layer, w); }
    int64_t head_dense_t() const { return half + head_dense(); }
    int64_t head_t() const { return half + head(); }
    int64_t total() const { return 2 * half; }
};

// What the kzv_stream_set_* calls hand a wave of slot-refill decoding.  The initialisers are the neutral values and kzv_stream_begin
// resets the whole by one assignment, so that no option leaks from one wave into the next.  (The n-best arrays live in the public
// kzv_stream_beam_state and are reset beside that assignment; the host copy of the suppress mask lives beside sdiv, for its lifetime.)
struct StreamWaveOpts {
    // alternatives of a greedy wave (kzv_stream_set_topk): candidates per position (0: off) and the caller's arrays [n_images, ld_alt]
    int topk = 0; int32_t* alt_ids = nullptr; float* alt_lp = nullptr; int64_t ld_alt = 0;
    // generation controls (kzv_stream_set_controls): on only while a control is not neutral; whether kzv_model::smask holds a mask
    bool ctl_on = false, mask_on = false;
    kzv_logits_controls ctl = {0, /* repetition_penalty */ 1.f, 0, 0, nullptr};
    // language-model fusion (kzv_stream_set_lm): on only while the weight is not zero; the struct is a copy, its tables are the
    // caller's device memory
    bool lm_on = false; float lm_weight = 0.f;
    kzv_ngram_lm lm = {};
    // forced prefixes (kzv_stream_set_prefix): on only while ld_prefix > 0; the tables are the caller's device memory
    bool pfx_on = false;
    const int64_t* pfx = nullptr; int64_t pfx_ld = 0; const int32_t* pfx_len = nullptr;
    float* pfx_lp = nullptr; int64_t pfx_lp_ld = 0;
};

#pragma GCC visibility pop       // the handle's type is the C ABI's (include/kzv.h): default visibility, as ever
// What of the handle is plain data (kzv_workspace_bytes plans on a copy of it); the device memory and graphs it owns follow in kzv_model
struct kzv_model_plain {
    kzv_config c;
    int np, Se, PD, He, Fe, Hd, Fd, V, Vp, Le, Ld;
    int npa = 0, Sa = 0, img_w = 0;   // ACTIVE geometry (kzv_set_image_width): img_w <= c.image_w, npa patches, Sa = npa + 1 tokens
    bool has_proj;
    bool long_seq = false;            // KZV_MODEL_LONG_SEQ: launches beyond 288 tokens take the streaming attention kernels
    std::vector<PEntry> table;
    int64_t total = 0;
    // parameters: the model-level linears (word: the tied LM head, its bias the head bias; ckv: cross-attention K/V of all decoder layers;
    // hd: the head's dense layer), the other offsets, the layers
    Lin patch, proj, word, ckv, hd;
    int64_t cls, pos, lnf_w, lnf_b, dpos, dtype, eln_w, eln_b, hln_w, hln_b;
    std::vector<EncLayerP> ep;
    std::vector<DecLayerP> dp;
    // bound state
    float* P = nullptr; float* G = nullptr; char* ws = nullptr; int64_t ws_bytes = 0;
    int B = 0, L = 0, T = 0, Ta = 0;
    int Be = 0;              // images the encoder states / cross-attention K/V currently hold (B after kzv_forward_loss; fewer after kzv_encode_images)
    bool bound = false, have_fwd = false, have_enc = false, train = false;
    // the decoder activations of a full kzv_forward_loss (train or not) are in the workspace: what kzv_cross_attention / kzv_score_tokens read
    bool have_dec = false;
    uint64_t seed = 0;
    const int64_t* labels = nullptr;
    // workspace pointers
    KzvCastDesc* d_desc = nullptr; int ndesc = 0, cast_tiles = 0;
    std::vector<KzvCastDesc> h_desc;
    bf16_t *patches, *enc_out, *proj_out, *crosskv, *xd0h, *hd_pre, *hd_ln, *dlogits;
    float *pe32, *x_last, *stf, *emb_sum, *emb_st, *xd0, *hd_gelu, *hd_st, *logits, *count, *loss_acc;
    int *posids, *err;
    std::vector<EncAct> ea;
    std::vector<DecAct> da;
    // backward scratch
    float *dx_e, *dx_d, *dsum_d;
    bf16_t *dy_e2;           // second dy_e (overlap mode 2: the fc2 weight gradient still reads dy_e while LayerNorm-2 backward writes its output)
    bf16_t *dy_e, *dbig_e, *dh_e, *dqkv_e, *dctx_e, *dpatch, *denc_out, *denc, *dckv, *dy_d, *dbig_d, *dqkv_d, *dctx_d, *dq_d, *dhln;
    bf16_t *dy_d2, *dy_d3;   // the decoder's three "dropout(linear)" gradients of a layer stay alive until its grouped weight-gradient launch
    std::vector<kzv_gemm_tn_args> wbatch;
    // weight-gradient GEMMs run on an internal side stream so they overlap the input-gradient chain on the
    // caller's stream (their tails and epilogues fill each other's idle workgroup slots)
    hipStream_t side = nullptr; hipEvent_t ev_fork = nullptr; hipEvent_t ev_done[4] = {nullptr, nullptr, nullptr, nullptr};
    bool pending[4] = {false, false, false, false}; bool use_side = false, join_each_segment = true;
    // generation path (kzv_decode_step): the geometry of the KV cache (kzv_model::kvc) and the row table in use (rt_cur = -1: identity)
    int kvB = 0, kvT = 0, rt_cur = -1;
    bool ckv_dec_ok = false;     // kzv_model::ckv_dec holds the images encoded last
    bool dec_pack_ok = false; DecPack pk;      // kzv_model::dec_pack is fresh; pk: where each matrix sits in it
    // generation from e4m3 decoder weights (kzv_set_decode_weights): the format asked for; kzv_model::dec_pack8 / dec_scale8 are fresh
    int dec_weights = KZV_DECODE_WEIGHTS_BF16;
    bool dec_pack8_ok = false;
    bool dhln_fused = false;     // the last training forward's head_ce launch already wrote dhln (the LM head's input gradient)
    float label_smoothing = 0.f; // kzv_set_label_smoothing: the loss of TRAINING forwards; evaluation forwards keep the plain NLL
    // kzv_set_focal_gamma / kzv_set_class_weights, TRAINING forwards only like label_smoothing: the focal exponent, and whether
    // kzv_model::class_w holds weights (the host copy is what kzv_get_class_weights returns); {W, S_w} of a step live at count + 4
    float focal_gamma = 0.f;
    int frozen_enc = 0;          // kzv_set_frozen_encoder_layers: backward segments > Le - frozen_enc launch nothing
    bool class_w_on = false;
    std::vector<float> class_w_h;
    int* d_t = nullptr;          // graph-replayed decode step (kzv_decode_step_graph): device-side step index
    // slot-refill decoding (kzv_stream_*): the images kzv_model::spool holds, the geometry kzv_model::sstate was laid out for, the slots'
    // state and logits inside it, the wave in progress
    int spool_images = 0, sstate_slots = 0, sstate_V = 0;
    kzv_stream_state sst = {}; float* slogits = nullptr; bool swave = false;
    // beam search on the slots (kzv_stream_begin_beams): beams per slot (0: the wave is greedy), the beam state, the ranking buffers
    int sbeams = 0;
    kzv_stream_beam_state sbst = {}; float* stop_lp = nullptr; int64_t* stop_ix = nullptr;
    StreamWaveOpts sopt;         // what the kzv_stream_set_* calls gave the wave in progress
    // the host copies of the divisor table and of the suppress mask, each kept for as long as the asynchronous copy to the device may
    // still read it (until the next kzv_stream_begin_beams / kzv_stream_set_controls writes it again)
    std::vector<float> sdiv;
    std::vector<uint32_t> smask_h;
    // fp8 weight path (kzv_set_fp8; BASELINE configs[4]): the encoder's QKV, fc1 and fc2 FORWARD GEMMs read e4m3 operands.
    // Weights: one e4m3 copy per matrix (Lin::q), quantised per output row from the fp32 master at kzv_model_sync_weights.  Activations:
    // LayerNorm writes an e4m3 copy of its output beside the bf16 one, quantised per token row (x8, x8_scale); the fc1 GELU
    // epilogue writes an e4m3 copy of the activation with a per-tensor multiplier (f8_q[layer]) derived from the largest |value|
    // the previous forward saw (f8_amax[layer]; "delayed scaling").  Backward and the output projection stay bf16.
    int fp8 = 0;
    KzvQuantDesc* d_qdesc = nullptr; int nqdesc = 0, qrows = 0;
    std::vector<KzvQuantDesc> h_qdesc;
    unsigned char *x8 = nullptr, *act8 = nullptr;
    float *x8_scale = nullptr, *f8_q = nullptr, *f8_amax = nullptr, *f8_rows = nullptr;
    int64_t f8_stride = 0;
    // mode 2: also the MLP's two INPUT-GRADIENT GEMMs (d fc2 with the DGELU epilogue, d fc1).  Transposed e4m3 weight copies
    // (Lin::qt, quantised per row from the bf16 transposed copies); the masked gradient rows arriving at fc2 come from the LayerNorm
    // backward above them as e4m3 with their own amax (dy8, dy8_scale); the gradient of the GELU input is quantised per row
    // in the DGELU epilogue with a multiplier from the bound ||dy row|| * max ||W2 column|| (rq / rqinv; f8_wnorm[layer]).
    unsigned char *dy8 = nullptr, *dbig8 = nullptr;
    float *dy8_scale = nullptr, *dy8_rq = nullptr, *dy8_rqinv = nullptr, *f8_wnorm = nullptr;
    bool side_ok = false;    // mode 2: set only inside the encoder-layer schedule (everything else stays on the caller's stream)
    int side_mode = 0;       // 0 off, 1 free-running wgrads, 2 wgrads only under the HBM-bound kernels (LayerNorm / attention backward)
};

// The handle: the plain part plus the device memory of the generation paths, which it owns (dev_buf.h: freed with the handle) and the
// captured graphs that hold pointers into it.  Graphs die before buffers: a graph handle has no destructor, so kzv_model_destroy calls
// drop_decode_graphs first and the buffers' destructors run after it; every reserve() that moves a buffer is followed by the same call.
struct kzv_model : kzv_model_plain {
    // KV cache of the generation path [2*Ld][B][T][Hd]; beam steps re-parent rows through the two row tables instead of copying it:
    // rowtab[x][b][j] = cache row holding key j of sequence b
    KzvDevBuf kvc, rowtab[2];
    // cross-attention K/V re-laid out for the generation steps ([layer][K|V][image][head][key][64]); rebuilt when the encoder ran
    KzvDevBuf ckv_dec;
    // the decoder's bf16 weights in MFMA fragment order (layout: DecPack), refreshed after every weight change; the e4m3 stream + row
    // scales of the linears the one-launch step reads (decode_fused.hip), built lazily while the format is e4m3 and refreshed alike
    KzvDevBuf dec_pack, dec_pack8, dec_scale8;
    // slot-refill decoding: the pool of cross-attention K/V in decode layout ([layer][K|V][pool image][head][key][64]), the slots' state
    // and logits (one allocation, sized by the bound batch)
    KzvDevBuf spool, sstate;
    // the device copy of a wave's suppress mask ((vocab + 31) / 32 words)
    KzvDevBuf smask;
    // the log-probability rows of a beam wave (kzv_stream_set_nbest with d_logprob): run_lp | fin_lp, fp32 [bound batch, max_len] each
    KzvDevBuf snbest;
    // the class weights of the training loss, fp32 [vocab] (kzv_set_class_weights)
    KzvDevBuf class_w;
    hipGraphExec_t dgraph[3] = {nullptr, nullptr, nullptr};          // one per row table in use: none, rowtab[0], rowtab[1]
    const void* dg_key[3][6] = {};
    int64_t dg_ld[3] = {0, 0, 0};
    hipGraphExec_t sgraph = nullptr;                                 // the wave's step
};

#pragma GCC visibility push(hidden)

// ---- what crosses the units --------------------------------------------------------------------------------------------
// model_train.cpp
KZV_LOCAL int forward(kzv_model* m, const float* px, const int64_t* labels, float* d_loss, float* d_logits, hipStream_t s,
                      bool run_encoder = true, int logits_pos = -1, int enc_batch = 0, bool run_decoder = true);
KZV_LOCAL int backward_decoder(kzv_model* m, hipStream_t s);
KZV_LOCAL int backward_enc_layer(kzv_model* m, int i, hipStream_t s);
KZV_LOCAL int backward_embed(kzv_model* m, hipStream_t s);
KZV_LOCAL int dec_chain_mode();         // KZV_DEC_CHAIN / kzv_set_dec_chain: 0, 1 or 2 (default)
KZV_LOCAL bool head_ce_mode();          // KZV_HEAD_CE / kzv_set_head_ce (default on)
// model_decode.cpp
KZV_LOCAL bool dec_pack_wanted(const kzv_model* m);
KZV_LOCAL int ensure_dec_pack(kzv_model* m, hipStream_t s);
KZV_LOCAL int ensure_dec_pack8(kzv_model* m, hipStream_t s);      // the e4m3 stream, where the next cached step would read it
KZV_LOCAL int decode_one_launch_mode(); // KZV_DECODE_ONE_LAUNCH / kzv_set_decode_one_launch (default on)
KZV_LOCAL bool reserve(kzv_model* m, KzvDevBuf& buf, size_t bytes);      // false: the allocation failed; a buffer that moved drops the graphs
KZV_LOCAL int ensure_kv_cache(kzv_model* m);
KZV_LOCAL int build_dec_pack8(kzv_model* m, hipStream_t s);
KZV_LOCAL int fused_common(kzv_model* m, KzvDecodeFused& a, bool e4m3, const char* who);
KZV_LOCAL int vocab_logits(kzv_model* m, bool fold_ln, float* d_logits, hipStream_t s);

// the captured step of a slot-refill wave holds the wave's outputs, counts and options: dropped when one of them changes
static inline void drop_stream_graph(kzv_model* m) {
    if (m->sgraph) { (void)hipGraphExecDestroy(m->sgraph); m->sgraph = nullptr; }
}
// a captured decode step holds pointers into the workspace, the caches and the pack: dropped whenever one of them moves
static inline void drop_decode_graphs(kzv_model* m) {
    for (int i = 0; i < 3; ++i) if (m->dgraph[i]) { (void)hipGraphExecDestroy(m->dgraph[i]); m->dgraph[i] = nullptr; }
    drop_stream_graph(m);
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

// dropout site ids (distinct hash keys per call site and layer)
enum { SITE_ENC_EMB = KZV_SITE_ENC_EMB, SITE_ENC_L = KZV_SITE_ENC_LAYER(0, 0), SITE_DEC_EMB = KZV_SITE_DEC_EMB, SITE_DEC_L = KZV_SITE_DEC_LAYER(0, 0) };
static inline uint32_t key(const kzv_model* m, uint32_t site) { return kzv_drop_key(m->seed, site); }
static inline float dp(const kzv_model* m, float p) { return m->train ? p : 0.f; }

// ---- Linear forward and input gradient ------------------------------------------------------------------------------------
// What a call adds to "C = A . W^T + bias" (forward) or "dX = dY . W" (input gradient); every field is optional.
struct LinOpts {
    const float* resid = nullptr;       // KZV_EPI_RESID: C += resid (row stride = ldc)
    void* aux = nullptr; int64_t ldaux = 0;   // GELU: the pre-activation written beside C; DGELU: read
    float drop_p = 0.f; uint32_t drop_key = 0;
    int n = 0;                          // the tied LM head only: the vocabulary padded to n columns (zeros / no store beyond lin.N)
    // fp8 path: A as e4m3 with one scale per row (the Lin's q copy multiplies it, qt in the input gradient) ...
    const unsigned char* a8 = nullptr; const float* a8_scale = nullptr;
    // ... and an e4m3 copy of C for the next GEMM: per-tensor multiplier + amax, or one multiplier per row
    unsigned char* c8 = nullptr; const float* c8_qscale = nullptr; float* c8_amax = nullptr; const float* c8_rowq = nullptr;
};

static inline int gemm_nt_call(const bf16_t* A, int64_t lda, const bf16_t* Bw, int64_t ldb, int M, int N, int K, int n_valid, const float* bias,
                               void* C, int64_t ldc, int epi, hipStream_t s, const LinOpts& o) {
    kzv_gemm_nt_args a;
    memset(&a, 0, sizeof(a));
    a.A = A; a.lda = lda; a.B = Bw; a.ldb = ldb;
    a.C = C; a.ldc = ldc; a.bias = bias; a.resid = o.resid; a.ldr = ldc; a.aux = o.aux; a.ldaux = o.ldaux;
    a.M = M; a.N = N; a.K = K; a.n_valid = n_valid; a.drop_p = o.drop_p; a.drop_key = o.drop_key;
    return kzv_gemm_nt(&a, epi, s);
}
// fp8 GEMM of the encoder: A e4m3 with one scale per row, W e4m3 with one scale per output row
static inline int gemm_fp8_call(const W8& w, int M, int N, int K, const float* bias, void* C, int64_t ldc, int epi, hipStream_t s, const LinOpts& o) {
    kzv_gemm_nt_fp8_args a;
    memset(&a, 0, sizeof(a));
    a.A = o.a8; a.lda = K; a.a_scale = o.a8_scale; a.B = w.w; a.ldb = K; a.b_scale = w.scale;
    a.C = C; a.ldc = ldc; a.bias = bias; a.resid = o.resid; a.ldr = ldc; a.aux = o.aux; a.ldaux = o.ldaux;
    a.c8 = o.c8; a.ldc8 = N; a.c8_qscale = o.c8_qscale; a.c8_amax = o.c8_amax; a.c8_rowq = o.c8_rowq;
    a.M = M; a.N = N; a.K = K; a.n_valid = N; a.drop_p = o.drop_p; a.drop_key = o.drop_key;
    return kzv_gemm_nt_fp8(&a, epi, s);
}

// C[M, N] = epi(A[M, K] . W^T + bias); with o.a8 the e4m3 operands (A is then unused)
static inline int lin_fwd(const kzv_model* m, const Lin& l, const bf16_t* A, int64_t lda, int M, void* C, int64_t ldc, int epi, hipStream_t s,
                          const LinOpts& o = {}) {
    if (o.a8) return gemm_fp8_call(l.q, M, l.N, l.K, m->P + l.b, C, ldc, epi, s, o);
    return gemm_nt_call(A, lda, l.h.w, l.K, M, o.n ? o.n : l.N, l.K, l.N, m->P + l.b, C, ldc, epi, s, o);
}
// dX[M, K] = epi(dY[M, N] . W)  (B operand = the transposed copy [K, ldt])
static inline int lin_dgrad(const kzv_model* m, const Lin& l, const bf16_t* dY, int64_t ldy, int M, void* dX, int64_t ldx, int epi, hipStream_t s,
                            const LinOpts& o = {}) {
    if (o.a8) return gemm_fp8_call(l.qt, M, l.K, l.N, nullptr, dX, ldx, epi, s, o);
    return gemm_nt_call(dY, ldy, l.h.wt, l.h.ldt, M, l.K, o.n ? o.n : l.N, l.K, nullptr, dX, ldx, epi, s, o);
}

// ---- LayerNorm ---------------------------------------------------------------------------------------------------------------
// gw / gb: the offsets of gamma and beta.  The defaults are the common case: every row normalised alike, no dropout.
struct LnFwdOpts {
    int seq = 1, drop_first = 0;        // rows per sequence; 1: the first row of each sequence (CLS) is left out of the output
    float drop_p = 0.f; uint32_t drop_key = 0;
    void* y8 = nullptr; float* y8_scale = nullptr;      // fp8 path: e4m3 copy of the output, one scale per row
};
static inline int ln_fwd(const kzv_model* m, const float* x, int64_t gw, int64_t gb, void* y16, float* y32, float* stats, int rows, int H, hipStream_t s,
                         const LnFwdOpts& o = {}) {
    return kzv_ln_fwd_ex(x, m->P + gw, m->P + gb, y16, y32, stats, rows, H, m->c.ln_eps, o.seq, o.drop_first, o.drop_p, o.drop_key, s, o.y8, o.y8_scale);
}
struct LnBwdOpts {
    int seq = 1, drop_first = 0;
    float drop_p = 0.f; uint32_t drop_key = 0;          // the dropout the forward applied to the LayerNorm's output
    bf16_t* out16 = nullptr; float out_drop_p = 0.f; uint32_t out_drop_key = 0;    // bf16 copy of dx under the mask of the Linear below
    const KzvLnBwdF8* f8 = nullptr;
};
// dx (+)= LayerNorm backward of dy (bf16, or fp32 with dy_is_f32); gamma / beta gradients go to G at the same offsets
static inline int ln_bwd(const kzv_model* m, const void* dy, int dy_is_f32, const float* x, const float* stats, int64_t gw, int64_t gb, float* dx,
                         int accumulate_dx, int rows, int H, hipStream_t s, const LnBwdOpts& o = {}) {
    return kzv_ln_bwd_ex(dy, dy_is_f32, x, stats, m->P + gw, dx, accumulate_dx, m->G + gw, m->G + gb, rows, H, o.seq, o.drop_first, o.drop_p, o.drop_key, s,
                         o.out16, o.out_drop_p, o.out_drop_key, o.f8);
}

#pragma GCC visibility pop
