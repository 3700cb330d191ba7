// Device-side pieces shared by the 256x256 GEMM kernels (gemm_nt256.hip, gemm_nt256p.hip, gemm_nt256f.hip, gemm_nt256h.hip,
// gemm_tn256.hip), each stated once.  Everything here has internal linkage: every unit compiles its own copy into its kernels.
#pragma once
#include "kzv_common.h"
#include "../../include/kzv.h"

namespace {

// LDS ring of the eight-wave gemm_nt kernels (gemm_nt256 / 256p / 256f and the gemm_nt phase of gemm_tn256's pair kernel): two K-tiles
// x four half-tiles.  gemm_nt256h.hip (72-KiB ring of three half-tile groups) and gemm_tn256.hip (64 tokens x 256 B half-tiles) keep
// their own geometry.
constexpr int NT256_HT_BYTES = 128 * 128;                      // half-tile: 128 rows x 128 B (64 bf16 / 128 e4m3)
constexpr int NT256_RING_BYTES = 8 * NT256_HT_BYTES;           // 128 KiB: all of gemm_nt256's LDS
constexpr int NT256_BUF_BYTES = 4 * NT256_HT_BYTES;            // ping-pong kernels (256, 256p, pair): a K-tile buffer = slots A-h0, A-h1, B-h0, B-h1
constexpr int KA0 = 0, KA1 = 1, KB0 = 2, KB1 = 3;              // (256f: A [buf][h] in the first 64 KiB of the ring, B [buf][h] in the second)
constexpr int NT256P_LDS_BYTES = NT256_RING_BYTES + 8 * 4096;  // persistent kernels (256p, 256f, pair): + one 4-KiB drain patch per wave = 160 KiB

// LDS-DMA, 16 B per lane: source = sbase (wave-uniform) + voff (per lane), destination = lds_dst + 16*lane.  lds_dst goes into M0 and
// stays there (kzv_common.h glds16_asm_soff_m0): a kernel that uses this issues EVERY LDS-DMA through it, and tools/check_m0.py
// checks on the ISA that the compiler has no M0 use of its own in such a kernel.
__device__ __forceinline__ void glds16_s(unsigned voff, const void* sbase, unsigned lds_dst) {
    asm volatile("s_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, %1" : : "v"(voff), "s"(sbase), "s"(lds_dst) : "memory");
}
// s_waitcnt vmcnt(N).  "n": the count is an immediate of the instruction, so it has to reach the asm as a compile-time constant.
template <int N> __device__ __forceinline__ void vmcnt() {
    static_assert(0 <= N && N <= 63, "vmcnt is a 6-bit field");
    asm volatile("s_waitcnt vmcnt(%0)" : : "n"(N) : "memory");
}
constexpr int cmin(int a, int b) { return a < b ? a : b; }

// vmcnt bookkeeping across a per-wave drain (the persistent kernels).  vmcnt counts this wave's VMEM operations in issue order (loads,
// stores, atomics and LDS-DMA count together and retire in order: MI355X_MICROARCH.md, `s_waitcnt vmcnt(N)`).  A wait that must retire
// an LDS-DMA load issued BEFORE the drain may leave outstanding every operation issued after that load: the kernel's usual count plus
// the D loads/stores of the drain.  D is only credited for interior tiles, where every row and column is stored (an edge tile skips
// some stores; crediting too few is merely conservative, crediting too many would be a race).
// D = VMEM operations one wave issues while draining an interior tile (32 four-column groups per lane):
template <int EPI, bool F8> constexpr int drain_ops() {
    // GELU*: two stores; RESID/DGELU: load + store; fp8: + the row scale (and the e4m3 copy of a GELU output)
    return ((EPI == KZV_EPI_BF16 || EPI == KZV_EPI_F32) ? 32 : 64) + (F8 ? ((EPI == KZV_EPI_GELU || EPI == KZV_EPI_DGELU) ? 64 : 32) : 0);
}

// Timeline stamps of the persistent kernels (dev builds with -DKZV_STAMPS, tools/dev/stamps_p.py, r4_half_stamps.py): thread 0 of a
// BF16-epilogue launch writes [block][16] u64 into p.aux: start, then (K loop end, drain end) per tile; slots 14 / 15 are the kernel's.
#ifdef KZV_STAMPS
#define KZV_STAMPS_BEGIN(EPI, tid, aux, bid) \
    unsigned long long* stp = ((EPI) == KZV_EPI_BF16 && (tid) == 0) ? (unsigned long long*)(aux) + (bid) * 16 : nullptr; \
    int stk = 0
#define KZV_STAMP() do { if (stp && stk < 15) stp[stk++] = __builtin_amdgcn_s_memrealtime(); } while (0)
#else
#define KZV_STAMPS_BEGIN(EPI, tid, aux, bid) do {} while (0)
#define KZV_STAMP() do {} while (0)
#endif

}  // namespace
