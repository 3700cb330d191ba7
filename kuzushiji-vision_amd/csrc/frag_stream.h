// The weight stream of the row-panel kernels (decode_fused.hip: the generation step, 4 linear waves; dec_rows.h: the training
// chains and their backward, 8 waves), stated once: a weight in MFMA FRAGMENT ORDER, read by each wave as one stream through a window of registers.
//
// Wp = the weight in fragment order (pack_frag_multi_kernel, frag_pack.hip): the 64 lanes' 16-byte pieces of (16-column block nb,
// 32-deep k-step ks) are 1 KiB of contiguous memory at ((nb * KS + ks) * 64 + lane) * 16 bytes, lane = (row nb * 16 + (lane & 15),
// columns ks * 32 + 8 (lane >> 4) .. + 7), so a wave-instruction is one contiguous KiB.  (Read from the row-major [N, K] copy, the 64
// lanes of a fragment are 64 separate 16-byte requests -- 16 rows x 4 pieces -- and the address coalescer, at one request per cycle,
// held the stream at 30 GB/s per CU: 13 us for the 393 KB of a QKV projection against 6.6.)
// With WS waves on the stream, wave w owns the column blocks w, w + WS, ...: fragment i of its CB x KS GEMM is (k-step i / CB, column
// block w + WS (i % CB)).  Slot i % window of the window is refilled right behind the MFMA that consumed it, with this GEMM's fragment
// i + window or, past its end, with the NEXT GEMM's first fragments (rows_gemm, chain_gemm: they differ in substance and stay with
// their kernels).
#pragma once
#include "kzv_common.h"

// the lane id, re-derived per phase: hipcc otherwise hoists every lane-derived offset of all phases out of the layer loop and spills them
__device__ __forceinline__ int opaque(int v) { asm volatile("" : "+v"(v)); return v; }
// Workgroup barrier for LDS hand-offs that leaves global loads in flight: __syncthreads() is a workgroup-scope release, and on gfx9
// that means s_waitcnt vmcnt(0) -- it would drain the streams at every phase boundary.  It orders LDS only: decode_fused.hip writes
// nothing to global memory that another wave of the launch reads, decoder_chain.hip waits for such stores itself (dec_chain_b_kernel).
__device__ __forceinline__ void wg_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

// where column block w of a weight with KS k-steps begins: wave w's fragment 0
template <int CB, int KS>
__device__ __forceinline__ const char* wave_frags(const bf16_t* Wp, int w) { return (const char*)(Wp + (int64_t)w * KS * 512); }
// wo = lane * 16
template <int CB, int KS, int WS>
__device__ __forceinline__ bf16x8 ld_frag(const char* wb, unsigned wo, int i) {
    const int ks = i / CB, c = i % CB;
    return *(const bf16x8*)(wb + ((int64_t)(WS * c) * KS + ks) * 1024 + wo);
}
// the first WIN fragments of a GEMM -> R[0 .. WIN)
template <int CB, int KS, int WS, int WIN, int N>
__device__ __forceinline__ void fill_window(bf16x8 (&R)[N], const char* wb, int lane) {
    static_assert(WIN <= N, "fill_window: window");
    const unsigned wo = (unsigned)lane * 16u;
#pragma unroll
    for (int i = 0; i < WIN; ++i) R[i] = ld_frag<CB, KS, WS>(wb, wo, i);
}
