// The decoder's weights -> MFMA fragment order (frag_stream.h has the layout): the B operands of the training chains (decoder_chain.hip,
// decoder_chain_bwd.hip, cross_entropy.hip's head) AND of the generation step (decode_fused.hip), refreshed by model_decode.cpp (for model_stream.cpp as well).
#include "kzv_common.h"
#include "../../include/kzv.h"
#include "kzv_host.h"
#include "kzv_kernels.h"

namespace {

// every decoder weight of the model -> fragment order, one launch
struct PackDesc { const uint4* src; uint4* dst; int N, K, t0, n_valid, ld, k_valid; };
constexpr int PACK_PER_LAUNCH = 96;        // 40-byte descriptors in the kernel argument block (4 KiB limit)
struct PackTable { PackDesc d[PACK_PER_LAUNCH]; int n; };
__global__ void pack_frag_multi_kernel(const PackTable tab, int total) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= total) return;
    int k = 0;
    while (k + 1 < tab.n && t >= tab.d[k + 1].t0) ++k;
    const PackDesc& d = tab.d[k];
    const int u = t - d.t0, lane = u & 63, f = u >> 6, KS = d.K / 32;
    const int nb = f / KS, ks = f - nb * KS;
    const int row = nb * 16 + (lane & 15), col = ks * 32 + (lane >> 4) * 8;      // rows beyond n_valid / columns beyond k_valid (the vocabulary's padding) pack as zeros
    d.dst[u] = (row < d.n_valid && col < d.k_valid) ? d.src[((int64_t)row * d.ld + col) / 8] : make_uint4(0, 0, 0, 0);
}

}  // namespace

int kzv_pack_frag_multi(const KzvPackJob* jobs, int n, hipStream_t s) {
    if (n < 1 || n > KZV_PACK_MAX_JOBS) return kzv_fail(KZV_E_ARG, "pack_frag_multi: 1..%d matrices", KZV_PACK_MAX_JOBS);
    for (int j0 = 0; j0 < n; j0 += PACK_PER_LAUNCH) {
        PackTable tab;
        int total = 0;
        const int cnt = n - j0 < PACK_PER_LAUNCH ? n - j0 : PACK_PER_LAUNCH;
        for (int i = 0; i < cnt; ++i) {
            const KzvPackJob& jb = jobs[j0 + i];
            if (jb.N % 16 || jb.K % 32) return kzv_fail(KZV_E_ARG, "pack_frag_multi: N %% 16, K %% 32");
            if (jb.ld % 8 || jb.k_valid % 8) return kzv_fail(KZV_E_ARG, "pack_frag_multi: ld %% 8, k_valid %% 8");
            tab.d[i] = PackDesc{(const uint4*)jb.src, (uint4*)jb.dst, jb.N, jb.K, total, jb.n_valid > 0 ? jb.n_valid : jb.N, jb.ld > 0 ? jb.ld : jb.K, jb.k_valid > 0 ? jb.k_valid : jb.K};
            total += jb.N * jb.K / 8;
        }
        tab.n = cnt;
        hipLaunchKernelGGL(pack_frag_multi_kernel, dim3((total + 255) / 256), dim3(256), 0, s, tab, total);
    }
    return kzv_check_launch("pack_frag_multi");
}
