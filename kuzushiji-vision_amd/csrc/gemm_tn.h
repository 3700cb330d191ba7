// Shared by the gemm_tn kernels -- gemm.hip (128x128 two-stage, single and grouped, and the dispatch) and gemm_tn256.hip (256x256:
// eight-phase, free-running, and the dgrad + wgrad pair kernel): launch parameters and the launchers' contracts.
#pragma once
#include "kzv_common.h"
#include "kzv_host.h"
#include "gemm_plan.h"

struct TnParams {
    const bf16_t* P; const bf16_t* Q; float* OUT; const void* zero16;
    int64_t ldp, ldq, ldo;
    int Mtok, N, K, n_store, splits, chunk;   // chunk = tokens per split (multiple of 64)
    float* dbias;                              // optional: dbias[n] += sum_t P[t][n]  (the nn.Linear bias gradient)
};

// ---- dispatch (gemm_plan.h) ----
KZV_LOCAL const KzvGemmSwitches& kzv_gemm_switches_tn();      // gemm_plan.cpp: the resolved switches, KZV_TN_CUS read again (as at every launch)
// gemm_plan.cpp: the argument validation of a kzv_gemm_tn call, no device needed; gemm.hip: the parameter block of a validated call
// (needs the zero page; splits / chunk come from the plan)
struct kzv_gemm_tn_args;
KZV_LOCAL int kzv_tn_validate(const kzv_gemm_tn_args* a, KzvTnShape* out);
KZV_LOCAL int kzv_tn_params(const kzv_gemm_tn_args* a, const KzvTnShape& sh, TnParams& p);
// gemm_tn256.hip: launches a TN256F / TN256 plan and the fold of its partial tiles (or leaves the fold pending, below).  1 = launched;
// 0 = no workspace could be had, nothing was launched: the caller falls back to the 128x128 kernel; < 0 = error (the fold of pending
// partial tiles it had to launch first failed: kzv_last_error has it).
KZV_LOCAL int kzv_tn256_launch(const TnParams& p, const KzvTnPlan& pl, hipStream_t s);

// While one of these is alive, kzv_tn256_launch leaves the fold of its partial tiles pending (each launch gets a workspace region of
// its own, up to 5); closing the outermost scope folds all of them in ONE launch on `stream` (the launches must be on it too;
// fold_queue.h).  close() returns that fold's code (KZV_OK for an inner scope); the destructor closes a scope nobody closed and drops
// the code, which is for paths that already return an error.
struct KzvTnFoldScope {
    explicit KzvTnFoldScope(hipStream_t stream);
    KzvTnFoldScope(const KzvTnFoldScope&) = delete;
    ~KzvTnFoldScope() { (void)close(); }
    int close();
    hipStream_t s; bool closed = false;
};

// gemm_tn256.hip: a layer's input-gradient GEMM (kzv_gemm_nt arguments, one-store epilogue) and its weight-gradient GEMM (kzv_gemm_tn
// arguments) as ONE launch when both take the 256x256 kernels: every workgroup runs its gemm_nt tiles and then a token range of one
// weight-gradient tile sized so that all workgroups finish together.  1 = launched, 0 = not taken (issue the two GEMMs separately), < 0 = error.
// Same results as the separate launches: the gemm_nt part bit for bit, the weight gradient up to the bf16 rounding of its partial tiles
// (the token splits differ).  KZV_PAIR=0 turns it off.
struct kzv_gemm_nt_args;
int kzv_gemm_pair_launch(const kzv_gemm_nt_args* na, int epilogue, const kzv_gemm_tn_args* ta, hipStream_t s);
