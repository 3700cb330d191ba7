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

int kzv_nt_strip() {
    static int v = -1000;
    if (v == -1000) {
        v = kzv_env_int("KZV_NT_STRIP", 3);
        if (v < 0 || v > 255) v = 0;
        if (kzv_env_int("KZV_BF16_DRAIN", 1) != 0) v |= 0x100;
    }
    return v;
}
namespace {
int nt256p_min_tiles() {
    static int v = -1;
    // 150 since the end of round 4 (384 before): the two 160-tile projections between encoder and decoder (41k x 256 x 768 forward, x 3072 input
    // gradient) and the decoder's 180-tile shapes run faster on fewer than 256 persistent workgroups than on the 128 x 128 kernel: step
    // 30.65 -> 30.58 ms, family +0.002 over five same-box alternations
    if (v < 0) v = kzv_env_int("KZV_NT256P_MIN_TILES", 150);
    return v;
}
}  // namespace

int kzv_nt256p_launch(const NtParams& p, int epilogue, hipStream_t s) {
    const int tilesN = (p.N + 255) / 256;
    const int tiles = ((p.M + 255) / 256) * tilesN;
    if (p.K < 128 || p.K % 128 || tiles < nt256p_min_tiles()) return 0;   // even number of K-tiles (odd: gemm_nt256.hip)
    if (!nt_dma_offsets_fit(p, 2)) return 0;
    int grid = tiles < kzv_device_cus() ? tiles : kzv_device_cus();
    { const int g = kzv_env_int("KZV_NT_GRID", 0); if (g > 0 && g < grid) grid = g; }   // dev: fewer persistent workgroups (two-chain experiment; read at every launch)
#define KZV_NT256P_CASE(E) case E: kzv_launch_lds<gemm_nt256p_kernel<E, false>>(dim3(grid), dim3(512), NT256P_LDS_BYTES, s, p, tiles, tilesN, kzv_nt_strip()); break;
    switch (epilogue) {
        KZV_NT256P_CASE(KZV_EPI_BF16) KZV_NT256P_CASE(KZV_EPI_F32) KZV_NT256P_CASE(KZV_EPI_GELU)
        KZV_NT256P_CASE(KZV_EPI_RESID) KZV_NT256P_CASE(KZV_EPI_DGELU) KZV_NT256P_CASE(KZV_EPI_GELU_F32)
        default: return 0;
    }
#undef KZV_NT256P_CASE
    return 1;
}

int kzv_nt256p_fp8_launch(const NtParams& p, int epilogue, hipStream_t s) {
    const int tilesN = (p.N + 255) / 256;
    const int tiles = ((p.M + 255) / 256) * tilesN;
    if (p.K < 256 || p.K % 256) return kzv_fail(KZV_E_ARG, "gemm_nt_fp8: K must be a multiple of 256 (an even number of 128-byte K-tiles)");
    if (!nt_dma_offsets_fit(p, 1)) return kzv_fail(KZV_E_ARG, "gemm_nt_fp8: operand panel beyond the 32-bit LDS-DMA offsets");
    const int grid = tiles < kzv_device_cus() ? tiles : kzv_device_cus();
#define KZV_NT256P8_CASE(E) case E: kzv_launch_lds<gemm_nt256p_kernel<E, true>>(dim3(grid), dim3(512), NT256P_LDS_BYTES, s, p, tiles, tilesN, kzv_nt_strip()); break;
    switch (epilogue) {
        KZV_NT256P8_CASE(KZV_EPI_BF16) KZV_NT256P8_CASE(KZV_EPI_GELU) KZV_NT256P8_CASE(KZV_EPI_RESID) KZV_NT256P8_CASE(KZV_EPI_DGELU)
        default: return kzv_fail(KZV_E_ARG, "gemm_nt_fp8: epilogue must be BF16, GELU, RESID or DGELU");
    }
#undef KZV_NT256P8_CASE
    return KZV_OK;
}
