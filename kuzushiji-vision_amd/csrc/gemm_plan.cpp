// The library's side of gemm_plan.h: the one KzvGemmSwitches of the process and its setters, the argument validation of kzv_gemm_nt /
// kzv_gemm_tn (no device needed), and the two queries that answer "what runs this shape?" without launching.
#include "kzv_host.h"
#include "../../include/kzv.h"
#include "gemm_plan.h"
#include "gemm_nt.h"
#include "gemm_tn.h"

static KzvGemmSwitches g_sw;
static int g_rows_scope = 0;

const KzvGemmSwitches& kzv_gemm_switches() { g_sw.resolve(kzv_env_int); return g_sw; }
const KzvGemmSwitches& kzv_gemm_switches_nt() { g_sw.resolve(kzv_env_int); g_sw.nt_grid = kzv_env_int("KZV_NT_GRID", 0); return g_sw; }
const KzvGemmSwitches& kzv_gemm_switches_tn() { g_sw.resolve(kzv_env_int); g_sw.tn_cus = kzv_env_int("KZV_TN_CUS", 0); return g_sw; }
KzvGemmEnv kzv_gemm_env() { return KzvGemmEnv{kzv_device_cus(), kzv_cu_reserve(), g_rows_scope}; }

KzvRowsScope::KzvRowsScope() { ++g_rows_scope; }
KzvRowsScope::~KzvRowsScope() { --g_rows_scope; }

// the setters: n < 0 puts the "not read yet" sentinel back where the header says so
extern "C" int kzv_set_nt_schedule(int n) { g_sw.nt_schedule = n < 0 ? -1 : (n & 3); return KZV_OK; }
extern "C" int kzv_set_nt_half_epilogues(int mask) { g_sw.nt_half_mask = mask; return KZV_OK; }
extern "C" int kzv_set_nt_half_stagger(int us) { g_sw.nth_stagger = us; return KZV_OK; }
extern "C" int kzv_set_rows_max_m(int n) {
    if (n < 0) return kzv_fail(KZV_E_ARG, "set_rows_max_m: >= 0");
    g_sw.rows_max_m = n;
    return KZV_OK;
}
extern "C" int kzv_set_tn_schedule(int n) { g_sw.tn_schedule = n < 0 ? -1 : (n != 0); return KZV_OK; }
extern "C" int kzv_set_pair(int n) { g_sw.pair = n < 0 ? -1 : (n != 0); return KZV_OK; }

int kzv_nt_validate(const kzv_gemm_nt_args* a, int epilogue, KzvNtShape* out) {
    if (!a || !a->A || !a->B || !a->C) return kzv_fail(KZV_E_ARG, "gemm_nt: null operand");
    if (a->M <= 0 || a->N <= 0 || a->K <= 0) return kzv_fail(KZV_E_ARG, "gemm_nt: empty shape");
    if (a->K % 64) return kzv_fail(KZV_E_ARG, "gemm_nt: K must be a multiple of 64");
    if (a->N % 4 || a->ldc % 4) return kzv_fail(KZV_E_ARG, "gemm_nt: N and ldc must be multiples of 4");
    if (a->lda % 8 || a->ldb % 8) return kzv_fail(KZV_E_ARG, "gemm_nt: lda/ldb must be multiples of 8 (16-byte rows)");
    if (((uintptr_t)a->A | (uintptr_t)a->B | (uintptr_t)a->C) & 15) return kzv_fail(KZV_E_ARG, "gemm_nt: operands must be 16-byte aligned");
    if (epilogue == KZV_EPI_RESID && (!a->resid || a->ldr % 4)) return kzv_fail(KZV_E_ARG, "gemm_nt: RESID needs resid, ldr%4==0");
    if ((epilogue == KZV_EPI_GELU || epilogue == KZV_EPI_DGELU || epilogue == KZV_EPI_GELU_F32) && (!a->aux || a->ldaux % 4)) return kzv_fail(KZV_E_ARG, "gemm_nt: GELU/DGELU need aux");
    *out = KzvNtShape{a->M, a->N, a->K, a->n_valid > 0 ? a->n_valid : a->N, a->lda, a->ldb, epilogue, 2};
    return KZV_OK;
}

int kzv_tn_validate(const kzv_gemm_tn_args* a, KzvTnShape* out) {
    if (!a || !a->P || !a->Q || !a->OUT) return kzv_fail(KZV_E_ARG, "gemm_tn: null operand");
    if (a->Mtok <= 0 || a->N <= 0 || a->K <= 0) return kzv_fail(KZV_E_ARG, "gemm_tn: empty shape");
    if (a->N % 8 || a->K % 8 || a->ldp % 8 || a->ldq % 8 || a->ldo % 4) return kzv_fail(KZV_E_ARG, "gemm_tn: N,K,ldp,ldq %8, ldo %4");
    if (((uintptr_t)a->P | (uintptr_t)a->Q | (uintptr_t)a->OUT) & 15) return kzv_fail(KZV_E_ARG, "gemm_tn: operands must be 16-byte aligned");
    *out = KzvTnShape{a->Mtok, a->N, a->K, a->n_store > 0 ? a->n_store : a->N, a->ldp, a->ldq, a->ldo};
    return KZV_OK;
}

extern "C" int kzv_gemm_nt_plan(const kzv_gemm_nt_args* a, int epilogue, int in_rows_scope, int cus, kzv_gemm_plan_info* out) {
    if (!out) return kzv_fail(KZV_E_ARG, "gemm_nt_plan: null out");
    KzvNtShape sh;
    KZV_TRY_RC(kzv_nt_validate(a, epilogue, &sh));
    const KzvGemmSwitches& sw = kzv_gemm_switches_nt();
    const KzvGemmEnv env{cus > 0 ? cus : kzv_device_cus(), kzv_cu_reserve(), in_rows_scope != 0};
    const KzvNtPlan pl = kzv_nt_plan(sh, sw, env);
    if (pl.rc != KZV_OK) return kzv_fail(pl.rc, "%s", pl.err);
    *out = kzv_gemm_plan_info{pl.kernel, pl.grid, pl.grid_y, pl.block, pl.tiles, 0, 0, kzv_pair_nt_ok(sh, sw, env)};
    return KZV_OK;
}

extern "C" int kzv_gemm_tn_plan(const kzv_gemm_tn_args* a, int cus, kzv_gemm_plan_info* out) {
    if (!out) return kzv_fail(KZV_E_ARG, "gemm_tn_plan: null out");
    KzvTnShape sh;
    KZV_TRY_RC(kzv_tn_validate(a, &sh));
    const KzvGemmSwitches& sw = kzv_gemm_switches_tn();
    const KzvGemmEnv env{cus > 0 ? cus : kzv_device_cus(), kzv_cu_reserve(), 0};
    const KzvTnPlan pl = kzv_tn_plan(sh, sw, env);
    // (the switch, the reserve and the device are the pair's whatever the epilogue of the other half)
    *out = kzv_gemm_plan_info{pl.kernel, pl.grid, 1, pl.block, pl.tiles, pl.splits, pl.chunk, kzv_pair_enabled(KZV_EPI_BF16, sw, env) && kzv_pair_tn_ok(sh, sw)};
    return KZV_OK;
}
