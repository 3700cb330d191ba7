// Host-side helpers shared by the launchers (error string, zero page, dropout thresholds).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "dev_buf.h"                                   // KzvDevBuf, KzvScratch: how device memory is owned

int kzv_fail(int code, const char* fmt, ...);          // records message, returns code
int kzv_check_launch(const char* what);                // hipGetLastError -> KZV_E_HIP
#define KZV_TRY_RC(expr) do { int rc__ = (expr); if (rc__ != KZV_OK) return rc__; } while (0)   // pass a failed check's code on (KZV_OK: include/kzv.h)
int kzv_cu_reserve();                                  // CUs left to concurrent collectives (kzv_set_cu_reserve / KZV_CU_RESERVE)
#define KZV_LOCAL __attribute__((visibility("hidden")))  // shared by the library's units, not part of its dynamic symbol table
KZV_LOCAL int kzv_device_cus();                        // compute units of the current device (read once; 256 if the query fails)
// An integer knob from the environment: atoi of the variable, `dflt` when it is unset.  One getenv per call: the caller keeps the
// result in a static of its own (a launcher runs ~180 times per training step), and a kzv_set_* that puts its global back to -1
// has the variable read again.
KZV_LOCAL int kzv_env_int(const char* name, int dflt);
const void* kzv_zero_page();                           // 4 KiB of device zeros (allocated once per process)
void kzv_drop_params(float p, unsigned* thr16, float* inv_keep);
extern "C" uint32_t kzv_drop_key(uint64_t seed, uint32_t site);

// Launch of a kernel that takes more dynamic LDS than the 64 KiB a kernel gets by default: the limit is raised once per kernel (the
// flag is a static of this template's instantiation, i.e. per kernel), then every call is a plain launch.  The caller checks the launch.
// kzv_launch_lds_max: a kernel whose launches ask for different amounts; the limit is the most any of them asks for.
template <auto Kernel, typename... Args>
inline void kzv_launch_lds_max(dim3 grid, dim3 block, int max_lds_bytes, int lds_bytes, hipStream_t s, const Args&... args) {
    static bool attr_done = false;
    if (!attr_done) { (void)hipFuncSetAttribute((const void*)Kernel, hipFuncAttributeMaxDynamicSharedMemorySize, max_lds_bytes); attr_done = true; }
    hipLaunchKernelGGL(Kernel, grid, block, lds_bytes, s, args...);
}
template <auto Kernel, typename... Args>
inline void kzv_launch_lds(dim3 grid, dim3 block, int lds_bytes, hipStream_t s, const Args&... args) {
    kzv_launch_lds_max<Kernel>(grid, block, lds_bytes, lds_bytes, s, args...);
}

// ---- optional per-launch HIP-event timing of the hot kernels (bench.py's roofline leg) -------------
// kind: 0 gemm_nt, 1 gemm_tn, 2 attn_fwd, 3 attn_bwd.  Off by default: zero cost when disabled.
struct KzvProfScope {
    int slot;
    hipStream_t s;
    KzvProfScope(int kind, double work, hipStream_t stream);
    ~KzvProfScope();
};
