// Model handle: create / destroy, parameter table, workspace plan, bind and the weight copies' refresh.  The training schedules are in
// model_train.cpp, the lockstep generation steps in model_decode.cpp, slot-refill decoding in model_stream.cpp; model_internal.h holds what
// the four share.
//
// Numeric policy (scripts/train_trocr.py:165-176 "bf16-mixed"): fp32 master weights and gradients, fp32
// residual stream / LayerNorm / softmax / loss, bf16 GEMM operands with fp32 accumulation.
#include "model_internal.h"

namespace {

int64_t add_param(kzv_model* m, const std::string& name, int64_t rows, int64_t cols) {
    const int64_t off = m->total;
    m->table.push_back({name, off, rows, cols});
    m->total += align_up(rows * cols, 64);
    return off;
}
// a Linear's weight [N, K] ("<name>.w") and bias [N] ("<name>.b"), in this order
void add_lin(kzv_model* m, Lin& l, const std::string& name, int64_t N, int64_t K) {
    l.N = (int)N; l.K = (int)K;
    l.w = add_param(m, name + ".w", N, K);
    l.b = add_param(m, name + ".b", N, 1);
}
void add_ln(kzv_model* m, int64_t& w, int64_t& b, const std::string& name, int64_t H) {
    w = add_param(m, name + ".w", H, 1);
    b = add_param(m, name + ".b", H, 1);
}

// MUST match kzv/params.py::param_table (tests/test_capi_cpu.py checks name/offset/shape equality)
void build_param_table(kzv_model* m) {
    const int He = m->He, Fe = m->Fe, Hd = m->Hd, Fd = m->Fd;
    add_lin(m, m->patch, "enc.patch", He, m->PD);
    m->cls = add_param(m, "enc.cls", He, 1);
    m->pos = add_param(m, "enc.pos", m->Se, He);
    m->ep.resize(m->Le);
    for (int i = 0; i < m->Le; ++i) {
        const std::string p = "enc." + std::to_string(i) + ".";
        EncLayerP& e = m->ep[i];
        add_ln(m, e.ln1w, e.ln1b, p + "ln1", He);
        add_lin(m, e.qkv, p + "qkv", 3 * He, He);
        add_lin(m, e.o, p + "o", He, He);
        add_ln(m, e.ln2w, e.ln2b, p + "ln2", He);
        add_lin(m, e.fc1, p + "fc1", Fe, He);
        add_lin(m, e.fc2, p + "fc2", He, Fe);
    }
    add_ln(m, m->lnf_w, m->lnf_b, "enc.lnf", He);
    if (m->has_proj) add_lin(m, m->proj, "proj", Hd, He);
    m->word.N = m->V; m->word.K = Hd;                 // the tied LM head: weight = the word embeddings, bias = head.bias (last entry)
    m->word.w = add_param(m, "dec.word", m->V, Hd);
    m->dpos = add_param(m, "dec.pos", m->c.max_pos, Hd);
    m->dtype = add_param(m, "dec.type", m->c.type_vocab, Hd);
    add_ln(m, m->eln_w, m->eln_b, "dec.emb_ln", Hd);
    add_lin(m, m->ckv, "dec.cross_kv", (int64_t)m->Ld * 2 * Hd, Hd);
    m->dp.resize(m->Ld);
    for (int i = 0; i < m->Ld; ++i) {
        const std::string p = "dec." + std::to_string(i) + ".";
        DecLayerP& d = m->dp[i];
        add_lin(m, d.qkv, p + "sa_qkv", 3 * Hd, Hd);
        add_lin(m, d.o, p + "sa_o", Hd, Hd);
        add_ln(m, d.ln1w, d.ln1b, p + "sa_ln", Hd);
        add_lin(m, d.cq, p + "ca_q", Hd, Hd);
        add_lin(m, d.co, p + "ca_o", Hd, Hd);
        add_ln(m, d.ln2w, d.ln2b, p + "ca_ln", Hd);
        add_lin(m, d.fc1, p + "fc1", Fd, Hd);
        add_lin(m, d.fc2, p + "fc2", Hd, Fd);
        add_ln(m, d.ln3w, d.ln3b, p + "out_ln", Hd);
    }
    add_lin(m, m->hd, "head.dense", Hd, Hd);
    add_ln(m, m->hln_w, m->hln_b, "head.ln", Hd);
    m->word.b = add_param(m, "head.bias", m->V, 1);
}

// ---- workspace bump allocator: pass 1 (base == nullptr) only measures ------------------------------
struct Bump {
    char* base; int64_t off = 0;
    template <class T> T* take(int64_t n) {
        off = align_up(off, 256);
        T* p = base ? (T*)(base + off) : nullptr;
        off += n * (int64_t)sizeof(T);
        return p;
    }
};

// the bf16 copy of a Linear's weight (and its transposed copy) + the cast job that refreshes them
void take_w(kzv_model_plain* m, Bump& b, Lin& l, bool need_t = true) {
    const int64_t N = l.N, K = l.K;
    W16& w = l.h;
    w.w = b.take<bf16_t>(N * K);
    w.ldt = align_up(N, 64);
    w.wt = need_t ? b.take<bf16_t>(K * w.ldt) : nullptr;
    KzvCastDesc d;
    d.src = m->P ? m->P + l.w : nullptr; d.dst = w.w; d.dstT = w.wt; d.rows = (int)N; d.cols = (int)K; d.ldT = w.ldt;
    d.tiles_c = (int)((K + 63) / 64);
    d.tile0 = m->cast_tiles;
    m->cast_tiles += (int)((N + 63) / 64) * d.tiles_c;
    m->h_desc.push_back(d);
}

// the e4m3 copy of the TRANSPOSED weight ([K, N], quantised per row from the bf16 transposed copy) + its quantisation job
void take_w8t(kzv_model_plain* m, Bump& b, Lin& l, float* normmax) {
    const int64_t rows = l.K, cols = l.N;
    l.qt.w = b.take<unsigned char>(rows * cols);
    l.qt.scale = b.take<float>(rows);
    KzvQuantDesc d{nullptr, l.qt.w, l.qt.scale, (int)rows, (int)cols, m->qrows, l.h.wt, l.h.ldt, normmax};
    m->h_qdesc.push_back(d);
    m->qrows += (int)rows;
}

// the e4m3 copy of the weight, quantised per output row from the fp32 master
void take_w8(kzv_model_plain* m, Bump& b, Lin& l) {
    const int64_t N = l.N, K = l.K;
    l.q.w = b.take<unsigned char>(N * K);
    l.q.scale = b.take<float>(N);
    m->h_qdesc.push_back(KzvQuantDesc{m->P ? m->P + l.w : nullptr, l.q.w, l.q.scale, (int)N, (int)K, m->qrows});
    m->qrows += (int)N;
}

// The ORDER of the take calls is the workspace layout (and the order of the cast / quantisation jobs): every offset depends on it.
int64_t plan(kzv_model_plain* m, char* base, int B, int L) {
    Bump b{base};
    const int T = L - 1;
    const int64_t Me = (int64_t)B * m->Se, Mp = (int64_t)B * m->np, Md = (int64_t)B * T;
    const int He = m->He, Fe = m->Fe, Hd = m->Hd, Fd = m->Fd;
    m->h_desc.clear(); m->cast_tiles = 0;
    // bf16 weight copies first: this whole region is zeroed at bind (transposed-copy padding stays zero)
    take_w(m, b, m->patch, false);
    for (EncLayerP& e : m->ep) { take_w(m, b, e.qkv); take_w(m, b, e.o); take_w(m, b, e.fc1); take_w(m, b, e.fc2); }
    if (m->has_proj) take_w(m, b, m->proj);
    take_w(m, b, m->word);
    take_w(m, b, m->ckv);
    for (DecLayerP& d : m->dp) { take_w(m, b, d.qkv); take_w(m, b, d.o); take_w(m, b, d.cq); take_w(m, b, d.co); take_w(m, b, d.fc1); take_w(m, b, d.fc2); }
    take_w(m, b, m->hd);
    m->ndesc = (int)m->h_desc.size();
    m->d_desc = b.take<KzvCastDesc>(m->ndesc);        // the zeroed region ends here (kzv_model_bind)
    m->h_qdesc.clear(); m->qrows = 0;
    if (m->fp8) {
        for (EncLayerP& e : m->ep) { take_w8(m, b, e.qkv); take_w8(m, b, e.fc1); take_w8(m, b, e.fc2); }
        if (m->fp8 >= 2) {
            m->f8_wnorm = b.take<float>(m->Le);
            for (int i = 0; i < m->Le; ++i) {
                take_w8t(m, b, m->ep[i].fc2, m->f8_wnorm ? m->f8_wnorm + i : nullptr);   // rows = W2 columns
                take_w8t(m, b, m->ep[i].fc1, nullptr);
            }
            m->dy8 = b.take<unsigned char>(Me * He); m->dbig8 = b.take<unsigned char>(Me * Fe);
            m->dy8_scale = b.take<float>(Me); m->dy8_rq = b.take<float>(Me); m->dy8_rqinv = b.take<float>(Me);
        }
        m->nqdesc = (int)m->h_qdesc.size();
        m->d_qdesc = b.take<KzvQuantDesc>(m->nqdesc);
        m->x8 = b.take<unsigned char>(Me * He); m->act8 = b.take<unsigned char>(Me * Fe);
        m->x8_scale = b.take<float>(Me);
        m->f8_q = b.take<float>(m->Le); m->f8_amax = b.take<float>(m->Le);
        m->f8_stride = Me; m->f8_rows = b.take<float>(Me * m->Le);
    }

    // scalars
    m->count = b.take<float>(64); m->loss_acc = m->count + 1; m->err = (int*)(m->count + 2);
    m->d_t = (int*)b.take<float>(64);
    m->posids = b.take<int>(Md);
    // encoder activations
    m->patches = b.take<bf16_t>(Mp * m->PD);
    m->pe32 = b.take<float>(Mp * He);
    m->ea.resize(m->Le);
    const int64_t lse_e = (int64_t)B * m->c.enc_heads * m->Se;
    for (int i = 0; i < m->Le; ++i) {
        EncAct& a = m->ea[i];
        a.x_in = b.take<float>(Me * He); a.x_mid = b.take<float>(Me * He);
        a.st1 = b.take<float>(Me * 2); a.st2 = b.take<float>(Me * 2); a.lse = b.take<float>(lse_e);
        a.ln1 = b.take<bf16_t>(Me * He); a.qkv = b.take<bf16_t>(Me * 3 * He); a.ctx = b.take<bf16_t>(Me * He);
        a.ln2 = b.take<bf16_t>(Me * He); a.pre = b.take<bf16_t>(Me * Fe); a.act = b.take<bf16_t>(Me * Fe);
    }
    m->x_last = b.take<float>(Me * He); m->stf = b.take<float>(Me * 2);
    m->enc_out = b.take<bf16_t>(Mp * He);
    m->proj_out = m->has_proj ? b.take<bf16_t>(Mp * Hd) : m->enc_out;
    // decoder activations
    const int64_t CK = (int64_t)m->Ld * 2 * Hd;
    m->crosskv = b.take<bf16_t>(Mp * CK);
    m->emb_sum = b.take<float>(Md * Hd); m->emb_st = b.take<float>(Md * 2);
    m->xd0 = b.take<float>(Md * Hd); m->xd0h = b.take<bf16_t>(Md * Hd);
    m->da.resize(m->Ld);
    const int64_t lse_d = (int64_t)B * m->c.dec_heads * T;
    for (int i = 0; i < m->Ld; ++i) {
        DecAct& a = m->da[i];
        a.s1 = b.take<float>(Md * Hd); a.x1 = b.take<float>(Md * Hd); a.s2 = b.take<float>(Md * Hd); a.x2 = b.take<float>(Md * Hd);
        a.s3 = b.take<float>(Md * Hd); a.x3 = b.take<float>(Md * Hd);
        a.st1 = b.take<float>(Md * 2); a.st2 = b.take<float>(Md * 2); a.st3 = b.take<float>(Md * 2);
        a.lse_sa = b.take<float>(lse_d); a.lse_ca = b.take<float>(lse_d);
        a.qkv = b.take<bf16_t>(Md * 3 * Hd); a.ctx = b.take<bf16_t>(Md * Hd); a.x1h = b.take<bf16_t>(Md * Hd);
        a.cq = b.take<bf16_t>(Md * Hd); a.cctx = b.take<bf16_t>(Md * Hd); a.x2h = b.take<bf16_t>(Md * Hd);
        a.pre = b.take<bf16_t>(Md * Fd); a.act = b.take<bf16_t>(Md * Fd); a.x3h = b.take<bf16_t>(Md * Hd);
    }
    m->hd_pre = b.take<bf16_t>(Md * Hd); m->hd_gelu = b.take<float>(Md * Hd); m->hd_st = b.take<float>(Md * 2);
    m->hd_ln = b.take<bf16_t>(Md * Hd);
    m->logits = b.take<float>(Md * m->Vp); m->dlogits = b.take<bf16_t>(Md * m->Vp);
    // backward scratch
    m->dx_e = b.take<float>(Me * He); m->dy_e = b.take<bf16_t>(Me * He); m->dy_e2 = b.take<bf16_t>(Me * He); m->dbig_e = b.take<bf16_t>(Me * Fe);
    m->dh_e = b.take<bf16_t>(Me * He); m->dqkv_e = b.take<bf16_t>(Me * 3 * He); m->dctx_e = b.take<bf16_t>(Me * He);
    m->dpatch = b.take<bf16_t>(Mp * He); m->denc_out = b.take<bf16_t>(Mp * He);
    m->denc = m->has_proj ? b.take<bf16_t>(Mp * Hd) : m->denc_out;
    m->dckv = b.take<bf16_t>(Mp * CK);
    m->dx_d = b.take<float>(Md * Hd); m->dsum_d = b.take<float>(Md * Hd);
    m->dy_d2 = b.take<bf16_t>(Md * Hd); m->dy_d3 = b.take<bf16_t>(Md * Hd);
    m->dy_d = b.take<bf16_t>(Md * Hd); m->dbig_d = b.take<bf16_t>(Md * Fd); m->dqkv_d = b.take<bf16_t>(Md * 3 * Hd);
    m->dctx_d = b.take<bf16_t>(Md * Hd); m->dq_d = b.take<bf16_t>(Md * Hd); m->dhln = b.take<bf16_t>(Md * Hd);
    if (kzv_dec_chain_supported(Hd, Fd))        // the segment path's per-layer gradient operands (2.8 KB per decoder row and layer)
        for (int i = 0; i < m->Ld; ++i) {
            DecAct& a = m->da[i];
            a.g_dy = b.take<bf16_t>(Md * Hd); a.g_dbig = b.take<bf16_t>(Md * Fd); a.g_dy2 = b.take<bf16_t>(Md * Hd);
            a.g_dq = b.take<bf16_t>(Md * Hd); a.g_dy3 = b.take<bf16_t>(Md * Hd); a.g_dqkv = b.take<bf16_t>(Md * 3 * Hd);
        }
    return align_up(b.off, 256);
}

}  // namespace

// ================================================================================================== C ABI
extern "C" int kzv_model_create(const kzv_config* cfg, kzv_model** out) { return kzv_model_create_ex(cfg, 0, out); }

extern "C" int kzv_model_create_ex(const kzv_config* cfg, unsigned flags, kzv_model** out) {
    if (!cfg || !out) return kzv_fail(KZV_E_ARG, "model_create: null");
    if (flags & ~KZV_MODEL_LONG_SEQ) return kzv_fail(KZV_E_ARG, "model_create: unknown flags 0x%x", flags);
    const kzv_config& c = *cfg;
    if (c.patch_h <= 0 || c.patch_w <= 0 || c.image_h % c.patch_h || c.image_w % c.patch_w)
        return kzv_fail(KZV_E_ARG, "model_create: image %dx%d not divisible by patch %dx%d", c.image_h, c.image_w, c.patch_h, c.patch_w);
    if (c.enc_heads <= 0 || c.dec_heads <= 0 || c.dec_hidden != 64 * c.dec_heads)
        return kzv_fail(KZV_E_ARG, "model_create: the decoder's head_dim must be 64 (hidden = 64 * heads)");
    if (c.enc_hidden % c.enc_heads || (c.enc_hidden / c.enc_heads) % 8 || c.enc_hidden / c.enc_heads > 128)
        return kzv_fail(KZV_E_ARG, "model_create: the encoder's head_dim must be a multiple of 8 up to 128 (64 and 96 take the MFMA attention kernels)");
    if (c.enc_ffn % 64 || c.dec_ffn % 64 || (c.channels * c.patch_h * c.patch_w) % 64 || c.patch_w % 8)
        return kzv_fail(KZV_E_ARG, "model_create: ffn sizes and C*ph*pw must be multiples of 64, patch_w of 8");
    const int np = (c.image_h / c.patch_h) * (c.image_w / c.patch_w);
    const int ehd = c.enc_hidden / c.enc_heads;
    if (np + 1 > KZV_ATTN_MAX_S) {
        if (!(flags & KZV_MODEL_LONG_SEQ))
            return kzv_fail(KZV_E_ARG, "model_create: %d patches + CLS exceed the 288-token attention kernels", np);
        if (ehd != 64 && ehd != 96)
            return kzv_fail(KZV_E_ARG, "model_create: %d patches + CLS exceed the 288-token attention kernels: the streaming kernels that take "
                                       "longer sequences serve encoder head_dim 64 and 96 only (this encoder's is %d)", np, ehd);
        if (np + 1 > KZV_ATTN_STREAM_MAX_S) return kzv_fail(KZV_E_ARG, "model_create: %d patches + CLS exceed the 4,097-token streaming attention kernels", np);
    }
    if (c.vocab < 8 || c.max_pos < 4 || c.type_vocab < 1 || c.pad_id < 0 || c.pad_id >= c.vocab)
        return kzv_fail(KZV_E_ARG, "model_create: bad vocabulary geometry");
    if (c.enc_layers < 1 || c.dec_layers < 1) return kzv_fail(KZV_E_ARG, "model_create: encoder and decoder need at least one layer each");
    kzv_model* m = new kzv_model();
    m->c = c;
    m->np = np; m->Se = np + 1; m->PD = c.channels * c.patch_h * c.patch_w;
    m->npa = np; m->Sa = np + 1; m->img_w = c.image_w;
    m->He = c.enc_hidden; m->Fe = c.enc_ffn; m->Hd = c.dec_hidden; m->Fd = c.dec_ffn;
    m->V = c.vocab; m->Vp = (int)align_up(c.vocab, 64); m->Le = c.enc_layers; m->Ld = c.dec_layers;
    m->has_proj = m->He != m->Hd;
    m->long_seq = (flags & KZV_MODEL_LONG_SEQ) != 0;
    m->pk = DecPack(m->Hd, m->Fd, m->Ld, m->V);
    build_param_table(m);
    *out = m;
    return KZV_OK;
}

extern "C" int kzv_model_destroy(kzv_model* m) {
    if (m) {
        if (m->side) (void)hipStreamDestroy(m->side);
        if (m->ev_fork) (void)hipEventDestroy(m->ev_fork);
        for (int i = 0; i < 4; ++i) if (m->ev_done[i]) (void)hipEventDestroy(m->ev_done[i]);
        drop_decode_graphs(m);       // graphs die before the buffers they point into, which `delete` frees
    }
    delete m;
    return KZV_OK;
}
extern "C" int kzv_param_count(const kzv_model* m) { return m ? (int)m->table.size() : 0; }
extern "C" int64_t kzv_param_total(const kzv_model* m) { return m ? m->total : 0; }

extern "C" int kzv_param_info(const kzv_model* m, int i, const char** name, int64_t* offset, int64_t* rows, int64_t* cols) {
    if (!m || i < 0 || i >= (int)m->table.size()) return kzv_fail(KZV_E_ARG, "param_info: index out of range");
    const PEntry& e = m->table[i];
    if (name) *name = e.name.c_str();
    if (offset) *offset = e.off;
    if (rows) *rows = e.rows;
    if (cols) *cols = e.cols;
    return KZV_OK;
}

static int check_batch(const kzv_model* m, int batch, int label_len) {
    if (batch <= 0) return kzv_fail(KZV_E_ARG, "batch must be positive");
    if (label_len < 2) return kzv_fail(KZV_E_ARG, "labels need at least 2 columns");
    if (label_len - 1 > KZV_ATTN_MAX_CAUSAL) return kzv_fail(KZV_E_ARG, "decoder length %d exceeds the 192-token attention kernels", label_len - 1);
    if ((int64_t)batch * m->Se * (int64_t)m->Fe >= (1ll << 31)) return kzv_fail(KZV_E_ARG, "batch too large for 32-bit element indices");
    return KZV_OK;
}

extern "C" int64_t kzv_workspace_bytes(const kzv_model* m, int batch, int label_len) {
    if (!m || check_batch(m, batch, label_len)) return -1;
    kzv_model_plain tmp = *m;   // plan() only writes pointer fields
    tmp.P = nullptr;
    return plan(&tmp, nullptr, batch, label_len);
}

extern "C" int kzv_model_bind(kzv_model* m, float* d_params, float* d_grads, void* d_workspace, int64_t workspace_bytes,
                              int batch, int label_len) {
    if (!m || !d_params || !d_workspace) return kzv_fail(KZV_E_ARG, "model_bind: null");
    KZV_TRY(check_batch(m, batch, label_len));
    if (m->long_seq) {       // the attention-dropout block index (kzv_common.h) is a 32-bit word: beyond it the masks would repeat
        const auto blocks = [](int64_t B, int64_t heads, int64_t Sq, int64_t Sk) { return B * heads * ((Sq + 3) / 4) * ((Sk + 3) / 4); };
        if (blocks(batch, m->c.enc_heads, m->Se, m->Se) > (1ll << 32) || blocks(batch, m->c.dec_heads, label_len - 1, m->np) > (1ll << 32))
            return kzv_fail(KZV_E_ARG, "model_bind: batch %d x %d tokens exceeds the 2^32 attention-dropout blocks of one launch", batch, m->Se);
    }
    if (((uintptr_t)d_params | (uintptr_t)d_grads | (uintptr_t)d_workspace) & 255) return kzv_fail(KZV_E_ARG, "model_bind: buffers must be 256-byte aligned");
    m->P = d_params; m->G = d_grads;
    const int64_t need = plan(m, (char*)d_workspace, batch, label_len);
    if (workspace_bytes < need) return kzv_fail(KZV_E_ARG, "model_bind: workspace %lld < required %lld", (long long)workspace_bytes, (long long)need);
    m->ws = (char*)d_workspace; m->ws_bytes = workspace_bytes;
    m->B = batch; m->L = label_len; m->T = label_len - 1; m->Ta = m->T;
    if (!kzv_zero_page()) return kzv_fail(KZV_E_HIP, "model_bind: zero page");
    // zero the bf16 weight region once (padding of transposed copies must read as 0), upload descriptors
    const int64_t wbytes = (char*)m->d_desc - (char*)d_workspace;
    if (hipMemset(d_workspace, 0, wbytes) != hipSuccess) return kzv_fail(KZV_E_HIP, "model_bind: memset");
    if (hipMemcpy(m->d_desc, m->h_desc.data(), sizeof(KzvCastDesc) * m->ndesc, hipMemcpyHostToDevice) != hipSuccess)
        return kzv_fail(KZV_E_HIP, "model_bind: descriptor upload");
    if (m->fp8) {
        if (hipMemcpy(m->d_qdesc, m->h_qdesc.data(), sizeof(KzvQuantDesc) * m->nqdesc, hipMemcpyHostToDevice) != hipSuccess)
            return kzv_fail(KZV_E_HIP, "model_bind: fp8 descriptor upload");
        const std::vector<float> ones((size_t)m->Le, 1.f);
        if (hipMemcpy(m->f8_q, ones.data(), sizeof(float) * m->Le, hipMemcpyHostToDevice) != hipSuccess ||
            hipMemset(m->f8_amax, 0, sizeof(float) * m->Le) != hipSuccess)
            return kzv_fail(KZV_E_HIP, "model_bind: fp8 scale state");
    }
    if (!m->side) {
        // KZV_SIDE_STREAM: 0 (default) = one stream; 1 = weight gradients free-running on a side stream: +3 % img/s
        // (7,180 -> 7,410), but the co-running kernels stretch each other (gemm_nt family 920 -> 715 TFLOP/s per launch),
        // so the per-kernel roofline accounting is only meaningful with it off; 2 = encoder weight gradients only under
        // the LayerNorm / attention backward kernels, every input-gradient GEMM joining the side stream first: the 120
        // cross-stream waits per step cost more than the overlap returns (6,400 img/s) -- kept for the record.
        m->side_mode = kzv_env_int("KZV_SIDE_STREAM", 0);
        m->use_side = m->side_mode != 0;
        if (m->use_side) {
            // (stream priorities make no measurable difference here: the range on this part is {0, -1})
            if (hipStreamCreateWithFlags(&m->side, hipStreamNonBlocking) != hipSuccess) return kzv_fail(KZV_E_HIP, "model_bind: side stream");
            if (hipEventCreateWithFlags(&m->ev_fork, hipEventDisableTiming) != hipSuccess) return kzv_fail(KZV_E_HIP, "model_bind: event");
            for (int i = 0; i < 4; ++i)
                if (hipEventCreateWithFlags(&m->ev_done[i], hipEventDisableTiming) != hipSuccess) return kzv_fail(KZV_E_HIP, "model_bind: event");
        }
    }
    // a captured decode step holds pointers INTO the workspace and the parameter buffer: none survives a rebind
    drop_decode_graphs(m);
    m->ckv_dec_ok = false; m->dec_pack_ok = false; m->dec_pack8_ok = false; m->swave = false;
    m->bound = true; m->have_fwd = false; m->have_enc = false; m->have_dec = false;
    return KZV_OK;
}

extern "C" int kzv_model_sync_weights(kzv_model* m, void* stream) {
    if (!m || !m->bound) return kzv_fail(KZV_E_STATE, "sync_weights: model not bound");
    KZV_TRY(kzv_cast_weights(m->d_desc, m->ndesc, m->cast_tiles, (hipStream_t)stream));
    m->dec_pack_ok = false; m->dec_pack8_ok = false;
    if (m->fp8) {
        if (m->fp8 >= 2 && hipMemsetAsync(m->f8_wnorm, 0, sizeof(float) * m->Le, (hipStream_t)stream) != hipSuccess)
            return kzv_fail(KZV_E_HIP, "sync_weights: memset");
        KZV_TRY(kzv_quant_rows(m->d_qdesc, m->nqdesc, m->qrows, (hipStream_t)stream));
    }
    return KZV_OK;
}

// fp8 weight path on / off; before kzv_model_bind (the workspace layout depends on it).
extern "C" int kzv_set_fp8(kzv_model* m, int mode) {
    if (!m) return kzv_fail(KZV_E_ARG, "set_fp8: null model");
    if (m->bound) return kzv_fail(KZV_E_STATE, "set_fp8: call before kzv_model_bind");
    if (mode < 0 || mode > 2) return kzv_fail(KZV_E_ARG, "set_fp8: mode 0 (bf16), 1 (e4m3 forward GEMMs of the encoder) or 2 (+ the MLP's input-gradient GEMMs)");
    if (mode && (m->He % 256 || m->Fe % 256))
        return kzv_fail(KZV_E_ARG, "set_fp8: encoder hidden %d and ffn %d must be multiples of 256 (128-byte K-tiles in pairs)", m->He, m->Fe);
    m->fp8 = mode;
    return KZV_OK;
}
extern "C" int kzv_get_fp8(const kzv_model* m) { return m ? m->fp8 : 0; }

// parity hook: the per-tensor multipliers the LAST forward quantised each layer's GELU output with -> d_out[enc_layers]
extern "C" int kzv_fp8_act_scales(const kzv_model* m, float* d_out, void* stream) {
    if (!m || !m->bound || !m->fp8 || !d_out) return kzv_fail(KZV_E_STATE, "fp8_act_scales: needs a bound model with the fp8 path on");
    if (hipMemcpyAsync(d_out, m->f8_q, sizeof(float) * m->Le, hipMemcpyDeviceToDevice, (hipStream_t)stream) != hipSuccess)
        return kzv_fail(KZV_E_HIP, "fp8_act_scales: copy");
    return KZV_OK;
}

extern "C" int kzv_set_image_width(kzv_model* m, int width) {
    if (!m) return kzv_fail(KZV_E_STATE, "set_image_width: null model");
    const kzv_config& c = m->c;
    if (width < c.patch_w || width > c.image_w || width % c.patch_w)
        return kzv_fail(KZV_E_ARG, "set_image_width: %d is not a multiple of the patch width %d within %d..%d", width, c.patch_w, c.patch_w, c.image_w);
    if (width != m->img_w) { m->have_fwd = false; m->have_enc = false; m->have_dec = false; }    // saved activations belong to the old geometry
    m->img_w = width;
    m->npa = (c.image_h / c.patch_h) * (width / c.patch_w);
    m->Sa = m->npa + 1;
    return KZV_OK;
}

extern "C" int kzv_set_active_length(kzv_model* m, int t_active) {
    if (!m || !m->bound) return kzv_fail(KZV_E_STATE, "set_active_length: model not bound");
    if (t_active < 1 || t_active > m->T) return kzv_fail(KZV_E_ARG, "set_active_length: must be in 1..%d", m->T);
    if (t_active != m->Ta) { m->have_fwd = false; m->have_dec = false; }   // saved activations belong to the old length
    m->Ta = t_active;
    return KZV_OK;
}

extern "C" int kzv_zero_grads(kzv_model* m, void* stream) {
    if (!m || !m->bound || !m->G) return kzv_fail(KZV_E_STATE, "zero_grads: no gradient buffer bound");
    if (hipMemsetAsync(m->G, 0, m->total * sizeof(float), (hipStream_t)stream) != hipSuccess) return kzv_fail(KZV_E_HIP, "zero_grads");
    return KZV_OK;
}
