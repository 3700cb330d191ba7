// The attention entry points of include/kzv.h and the ONE dispatch behind them: which kernel file serves a call, what each refuses
// (code and message), and the launch of a chosen implementation.  The kernel files (attention.hip, attention_d96.hip,
// attention_generic.hip, attention_stream.hip) keep their kernels and one internal launch function each (attention_common.h);
// they trust their arguments.  Every caller decides once, then launches: a call is validated once.
#include "attention_common.h"

namespace {

// what the head_dim-64 whole-head kernels refuse
int check64(const kzv_attn_args* a, bool bwd) {
    if (!a || !a->Q || !a->K || !a->V || !a->O) return kzv_fail(KZV_E_ARG, "attn: null operand");
    if (a->Sq <= 0 || a->Sk <= 0 || a->Sq > KZV_ATTN_MAX_S || a->Sk > KZV_ATTN_MAX_S) return kzv_fail(KZV_E_ARG, "attn: Sq/Sk must be in 1..288");
    if (a->mode == 1 && a->Sq > KZV_ATTN_MAX_CAUSAL) return kzv_fail(KZV_E_ARG, "attn: causal mode is built for <= 192 tokens");
    if (a->mode == 1 && (!a->ids || a->Sq != a->Sk)) return kzv_fail(KZV_E_ARG, "attn: causal mode needs ids and Sq == Sk");
    if (a->mode != 0 && a->mode != 1) return kzv_fail(KZV_E_ARG, "attn: unknown mode");
    if ((a->ldq | a->ldk | a->ldv | a->ldo) % 8) return kzv_fail(KZV_E_ARG, "attn: row strides must be multiples of 8");
    if (bwd && (!a->dO || !a->dQ || !a->dK || !a->dV || !a->LSE)) return kzv_fail(KZV_E_ARG, "attn_bwd: null gradient operand");
    return KZV_OK;
}

// what the head_dim-96 whole-head kernels take (anything else with that head_dim is the VALU kernel's)
bool takes96(const kzv_attn_args* a) {
    return a->head_dim == 96 && a->mode == 0 && a->Sq >= 1 && a->Sq <= KZV_ATTN_MAX_S && a->Sk >= 1 && a->Sk <= KZV_ATTN_MAX_S;
}

// what the VALU kernel (attention_generic.hip) refuses
int kzv_attn_generic_check(const kzv_attn_args* a, int D) {
    if (a->mode != 0) return kzv_fail(KZV_E_ARG, "attn: the causal / key-padding mode exists for head_dim 64 only");
    if (D < 8 || D > 128 || D % 8) return kzv_fail(KZV_E_ARG, "attn: head_dim must be a multiple of 8 in 8..128 (got %d)", D);
    if (a->Sq <= 0 || a->Sk <= 0 || a->Sk > KZV_ATTN_VALU_MAX_SK) return kzv_fail(KZV_E_ARG, "attn (generic head_dim): Sk must be in 1..512");
    if (kzv_attn_generic_lds(D, a->Sk) > 160 * 1024) return kzv_fail(KZV_E_ARG, "attn (generic head_dim): %d keys x head_dim %d do not fit the 160 KiB LDS", a->Sk, D);
    return KZV_OK;
}

int head_dim_of(const kzv_attn_args* a, int impl) {
    return impl == KZV_ATTN_MFMA64 || impl == KZV_ATTN_STREAM64 ? 64 : impl == KZV_ATTN_MFMA96 || impl == KZV_ATTN_STREAM96 ? 96 : a->head_dim;
}

}  // namespace

// what the streaming kernels refuse (kzv_attn_stream_fwd / _bwd, kzv_attn_impl_ex)
int kzv_attn_stream_check(const kzv_attn_args* a, bool bwd) {
    if (!a || !a->Q || !a->K || !a->V || !a->O) return kzv_fail(KZV_E_ARG, "attn_stream: null operand");
    if (a->head_dim != 0 && a->head_dim != 64 && a->head_dim != 96) return kzv_fail(KZV_E_ARG, "attn_stream: head_dim must be 64 or 96");
    if (a->mode != 0) return kzv_fail(KZV_E_ARG, "attn_stream: only mode 0 (no mask)");
    if (a->Sq < 1 || a->Sk < 1 || a->Sq > KZV_ATTN_STREAM_MAX_S || a->Sk > KZV_ATTN_STREAM_MAX_S) return kzv_fail(KZV_E_ARG, "attn_stream: Sq/Sk must be in 1..4097");
    if (a->B < 1 || a->heads < 1 || (int64_t)a->B * a->heads * (((a->Sq > a->Sk ? a->Sq : a->Sk) + 63) / 64) >= (1ll << 31))
        return kzv_fail(KZV_E_ARG, "attn_stream: B and heads must be positive and the grid within 2^31 workgroups");
    if ((a->ldq | a->ldk | a->ldv | a->ldo) % 8) return kzv_fail(KZV_E_ARG, "attn: row strides must be multiples of 8");
    if (bwd && (!a->dO || !a->dQ || !a->dK || !a->dV || !a->LSE)) return kzv_fail(KZV_E_ARG, "attn_stream_bwd: null gradient operand");
    return KZV_OK;
}

// Which kernels serve a call (include/kzv.h): head_dim 0 / 64 -> attention.hip; head_dim 96, mode 0, Sq and Sk in 1..288 ->
// attention_d96.hip; the other head dims the VALU kernel takes -> attention_generic.hip.  Arguments a launch would refuse give its
// error code and message.  The launches dispatch through this, so the report and the launch cannot disagree.
extern "C" int kzv_attn_impl(const kzv_attn_args* a, int bwd) {
    if (a && a->head_dim != 0 && a->head_dim != 64) {
        if (!bwd && (!a->Q || !a->K || !a->V || !a->O)) return kzv_fail(KZV_E_ARG, "attn: null operand");
        if (bwd && (!a->Q || !a->K || !a->V || !a->O || !a->dO || !a->dQ || !a->dK || !a->dV || !a->LSE)) return kzv_fail(KZV_E_ARG, "attn_bwd: null operand");
        if ((a->ldq | a->ldk | a->ldv | a->ldo) % 8) return kzv_fail(KZV_E_ARG, "attn: row strides must be multiples of 8");
        if (takes96(a)) return KZV_ATTN_MFMA96;
        if (int rc = kzv_attn_generic_check(a, a->head_dim)) return rc;
        return KZV_ATTN_VALU;
    }
    if (int rc = check64(a, bwd != 0)) return rc;
    return KZV_ATTN_MFMA64;
}

// With KZV_MODEL_LONG_SEQ the calls the whole-head kernels cannot take (head_dim 0 / 64 / 96, mode 0, Sq or Sk above 288) go to the
// streaming kernels; everything else is kzv_attn_impl's answer, so a short launch of a long-sequence model is unchanged.
extern "C" int kzv_attn_impl_ex(const kzv_attn_args* a, int bwd, unsigned flags) {
    if ((flags & KZV_MODEL_LONG_SEQ) && a && a->mode == 0 && (a->head_dim == 0 || a->head_dim == 64 || a->head_dim == 96) &&
        (a->Sq > KZV_ATTN_MAX_S || a->Sk > KZV_ATTN_MAX_S)) {
        if (int rc = kzv_attn_stream_check(a, bwd != 0)) return rc;
        return a->head_dim == 96 ? KZV_ATTN_STREAM96 : KZV_ATTN_STREAM64;
    }
    return kzv_attn_impl(a, bwd);
}

int kzv_attn_launch(const kzv_attn_args* a, int impl, bool bwd, hipStream_t s) {
    KzvProfScope prof(bwd ? 3 : 2, (bwd ? 10.0 : 4.0) * a->B * a->heads * (double)a->Sq * a->Sk * head_dim_of(a, impl), s);
    switch (impl) {
    case KZV_ATTN_MFMA64: return kzv_attn_mfma64(a, bwd, s);
    case KZV_ATTN_MFMA96: return kzv_attn_d96(a, bwd, s);
    case KZV_ATTN_VALU: return kzv_attn_generic(a, a->head_dim, bwd, s);
    case KZV_ATTN_STREAM64:
    case KZV_ATTN_STREAM96: return kzv_attn_stream(a, bwd, s);
    }
    return kzv_fail(KZV_E_ARG, "attn: unknown implementation %d", impl);
}

// never the streaming kernels: a caller that wants them asks for them (below) or decides through kzv_attn_impl_ex (model.cpp)
extern "C" int kzv_attn_fwd(const kzv_attn_args* a, void* stream) {
    const int impl = kzv_attn_impl(a, 0);
    return impl < 0 ? impl : kzv_attn_launch(a, impl, false, (hipStream_t)stream);
}

extern "C" int kzv_attn_bwd(const kzv_attn_args* a, void* stream) {
    const int impl = kzv_attn_impl(a, 1);
    return impl < 0 ? impl : kzv_attn_launch(a, impl, true, (hipStream_t)stream);
}

// always the streaming kernels, also at 288 tokens and below
extern "C" int kzv_attn_stream_fwd(const kzv_attn_args* a, void* stream) {
    if (int rc = kzv_attn_stream_check(a, false)) return rc;
    return kzv_attn_launch(a, a->head_dim == 96 ? KZV_ATTN_STREAM96 : KZV_ATTN_STREAM64, false, (hipStream_t)stream);
}

extern "C" int kzv_attn_stream_bwd(const kzv_attn_args* a, void* stream) {
    if (int rc = kzv_attn_stream_check(a, true)) return rc;
    return kzv_attn_launch(a, a->head_dim == 96 ? KZV_ATTN_STREAM96 : KZV_ATTN_STREAM64, true, (hipStream_t)stream);
}
