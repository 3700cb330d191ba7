// gemm_nt, persistent 256x256 eight-phase kernel for gfx950 (MI355X): the kernel (body and header comment: gemm_nt256p_body.h) and its
// bf16 and fp8 launchers.
#include "kzv_common.h"
#include "../../include/kzv.h"
#include "kzv_host.h"
#include "gemm_nt.h"
#include "gemm_nt256p_body.h"

namespace {

template <int EPI, bool F8>
__global__ __launch_bounds__(512) void gemm_nt256p_kernel(const NtParams p, const int tiles, const int tilesN, const int strip_in) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    nt256p_body<EPI, F8>(p, tiles, tilesN, strip_in, (int)blockIdx.x, (int)gridDim.x, smem);
}

}  // namespace

void kzv_nt256p_launch(const NtParams& p, const KzvNtPlan& pl, hipStream_t s) {
#define KZV_NT256P_CASE(E) case E: kzv_launch_lds<gemm_nt256p_kernel<E, false>>(dim3(pl.grid), dim3(512), NT256P_LDS_BYTES, s, p, pl.tiles, pl.tilesN, pl.strip); break;
    switch (pl.epilogue) {
        KZV_NT256P_CASE(KZV_EPI_BF16) KZV_NT256P_CASE(KZV_EPI_F32) KZV_NT256P_CASE(KZV_EPI_GELU)
        KZV_NT256P_CASE(KZV_EPI_RESID) KZV_NT256P_CASE(KZV_EPI_DGELU) KZV_NT256P_CASE(KZV_EPI_GELU_F32)
    }
#undef KZV_NT256P_CASE
}

void kzv_nt256p_fp8_launch(const NtParams& p, const KzvNtPlan& pl, hipStream_t s) {
#define KZV_NT256P8_CASE(E) case E: kzv_launch_lds<gemm_nt256p_kernel<E, true>>(dim3(pl.grid), dim3(512), NT256P_LDS_BYTES, s, p, pl.tiles, pl.tilesN, pl.strip); break;
    switch (pl.epilogue) {
        KZV_NT256P8_CASE(KZV_EPI_BF16) KZV_NT256P8_CASE(KZV_EPI_GELU) KZV_NT256P8_CASE(KZV_EPI_RESID) KZV_NT256P8_CASE(KZV_EPI_DGELU)
    }
#undef KZV_NT256P8_CASE
}
