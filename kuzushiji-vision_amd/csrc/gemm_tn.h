// Shared by the gemm_tn kernels -- gemm.hip (128x128 two-stage, single and grouped, and the dispatch) and gemm_tn256.hip (256x256:
// eight-phase, free-running, and the dgrad + wgrad pair kernel): launch parameters and the launchers' contracts.
#pragma once
#include "kzv_common.h"

struct TnParams {
    const bf16_t* P; const bf16_t* Q; float* OUT; const void* zero16;
    int64_t ldp, ldq, ldo;
    int Mtok, N, K, n_store, splits, chunk;   // chunk = tokens per split (multiple of 64)
    float* dbias;                              // optional: dbias[n] += sum_t P[t][n]  (the nn.Linear bias gradient)
};

// gemm_tn256.hip's twin of nt_dma_offsets_fit (gemm_nt.h): a 64-token stage of P and of Q within the 32-bit per-lane LDS-DMA offsets
inline bool tn_dma_offsets_fit(const TnParams& p) {
    return (uint64_t)64 * (uint64_t)p.ldp * 2 + (uint64_t)p.N * 2 <= 0xffffffffull && (uint64_t)64 * (uint64_t)p.ldq * 2 + (uint64_t)p.K * 2 <= 0xffffffffull;
}

// gemm_tn256.hip: returns 1 when it took the launch (p.splits / p.chunk are chosen inside), 0 when the shape is left
// to the 128x128 kernel, < 0 = error (the fold of pending partial tiles it had to launch first failed: kzv_last_error has it).
int kzv_tn256_launch(const TnParams& p, hipStream_t s);
// gemm.hip: validation of a kzv_gemm_tn call and its kernel parameter block (splits / chunk are the launcher's)
struct kzv_gemm_tn_args;
int kzv_tn_params(const kzv_gemm_tn_args* a, TnParams& p);

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
struct kzv_gemm_nt_args; struct kzv_gemm_tn_args;
int kzv_gemm_pair_launch(const kzv_gemm_nt_args* na, int epilogue, const kzv_gemm_tn_args* ta, hipStream_t s);
