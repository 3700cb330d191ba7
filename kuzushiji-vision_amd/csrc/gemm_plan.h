// GEMM dispatch, as a host-only header without a HIP include: which kernel runs a kzv_gemm_nt / kzv_gemm_tn call, on what
// grid and with what token splits, is decided HERE, once, from plain integers -- so a plain C++ program asks the same functions
// (tests/host/gemm_plan_main.cpp) and the library answers "what runs this shape?" without launching (kzv_gemm_nt_plan, kzv_gemm_tn_plan).
// The launchers (gemm*.hip) take a plan and launch it; every gate, threshold and switch default of the GEMM family is stated in this file only.
#pragma once
#include <stdint.h>
#include <vector>
#include "../../include/kzv.h"

#pragma GCC visibility push(hidden)

// ---- the tuning switches ---------------------------------------------------------------------------------------------------------
// An integer from the environment: atoi of the variable, `dflt` when it is unset (kzv_env_int; the test program passes a fake).
typedef int (*KzvEnvInt)(const char* name, int dflt);

// Every GEMM switch of the library.  A field holds its value once read; the sentinel in its initialiser (negative unless noted) means
// "not read yet": resolve() reads those, so a kzv_set_* that writes the sentinel back has the environment read again, and an
// environment value that is itself negative is read again at every plan (as the statics this struct replaces did).
struct KzvGemmSwitches {
    int nt_schedule = -1;         // bit 0: KZV_NT_FREE (0), the persistent kernel's K loop free-running (gemm_nt256f.hip); bit 1: KZV_NT_HALF (0), the
                                  // epilogues of nt_half_mask on the four-wave 256x128 kernel (gemm_nt256h.hip).  kzv_set_nt_schedule
    int nt_half_mask = -1;        // KZV_NT_HALF_EPIS (0x3f): 1 << KZV_EPI_*.  kzv_set_nt_half_epilogues
    int nt256p = -1;              // KZV_NT256P (1): the persistent kernels at all
    int nt256p_gelu = -1;         // KZV_NT256P_GELU (0): dev knob, the two-store GELU epilogues on the persistent kernels too (A/B; default off)
    int nth_max_k = -1;           // KZV_NTH_MAX_K (1 << 30): the four-wave kernel's K loop is latency-bound (three-group ring): it pays only where the
                                  // drain is a large part of a tile
    // KZV_NT256P_MIN_TILES feeds TWO fields with different defaults: the eight-phase persistent kernel from 150 tiles, the free-running
    // one from 384 (set, the variable moves both).  150 since the end of round 4 (384 before): the two 160-tile projections between
    // encoder and decoder (41k x 256 x 768 forward, x 3072 input gradient) and the decoder's 180-tile shapes run faster on fewer than
    // 256 persistent workgroups than on the 128 x 128 kernel: step 30.65 -> 30.58 ms, family +0.002 over five same-box alternations
    int nt256p_min_tiles = -1, nt256f_min_tiles = -1;
    int nt256_min_tiles = -1;     // KZV_NT256_MIN_TILES (384): below ~1.5 rounds of the 256 CUs the 128x128 kernel (4x the tiles, 2 workgroups per CU) fills the chip better
    int nt256h_min_tiles = -1;    // KZV_NT256H_MIN_TILES (768), in tiles of 256x128
    int nth_stagger = -1;         // KZV_NTH_STAGGER (8): how late the second workgroup of a CU starts, ~us.  kzv_set_nt_half_stagger
    int nt_strip = -1000;         // KZV_NT_STRIP (3; outside 0..255: 0) in bits 0..7, KZV_BF16_DRAIN (1) in bit 8.  Sentinel -1000
    int rows_max_m = -1;          // KZV_ROWS_MAX_M (0): the few-rows kernel outside a KzvRowsScope.  kzv_set_rows_max_m
    int tn_schedule = -1;         // KZV_TN_FREE (1): free-running stages (+10..13 % per launch, same-box A/B, bit-identical partial tiles).  kzv_set_tn_schedule
    // 9: the 768 x 768 outputs (attention output projection, patch embedding) take the 256x256 kernel too -- 28 token splits each,
    // 83 -> ~70 us against the 128 x 128 kernel (-0.13 ms per step, same-box A/B; round 2's threshold was 24)
    int tn256_min_tiles = -1;     // KZV_TN256_MIN_TILES (9)
    // default OFF: measured on the step's four encoder pairs (tools/dev/r4_pair.py, same-box A/B): -23 us per layer at best (one kernel
    // boundary per pair), +0.4 % img/s on the whole step -- and NO gain from sizing the token ranges to the gemm_nt tile counts (the
    // workgroups that leave the gemm_nt phase early then run their weight-gradient stages beside the others' gemm_nt tiles, and the
    // two loops slow each other as they do on two streams).  DESIGN.md section 8.
    int pair = -1;                // KZV_PAIR (0).  kzv_set_pair
    int pair_r = -2;              // KZV_PAIR_R (-1: none): overrides the pair plan's stage ratio, x 0.01.  Sentinel -2
    int tn_minsteps = -1;         // KZV_TN_MINSTEPS (16): reduction steps per workgroup of the 128x128 weight-gradient kernel, at least
    int tn_blocks = -1;           // KZV_TN_BLOCKS (512): its workgroup budget, one resident round
    // read at EVERY launch (the dev tools of round 5 change them between launches of one process): the callers below refresh them
    int nt_grid = 0;              // KZV_NT_GRID (0): fewer persistent workgroups (two-chain experiment)
    int tn_cus = 0;               // KZV_TN_CUS (0): fewer CUs for the 256x256 weight gradient (two-stream experiment)

    void resolve(KzvEnvInt env) {
        if (nt_schedule < 0) { nt_schedule = env("KZV_NT_FREE", 0) != 0; if (env("KZV_NT_HALF", 0)) nt_schedule |= 2; }
        if (nt_half_mask < 0) nt_half_mask = env("KZV_NT_HALF_EPIS", 0x3f);
        if (nt256p < 0) nt256p = env("KZV_NT256P", 1);
        if (nt256p_gelu < 0) nt256p_gelu = env("KZV_NT256P_GELU", 0);
        if (nth_max_k < 0) nth_max_k = env("KZV_NTH_MAX_K", 1 << 30);
        if (nt256p_min_tiles < 0) nt256p_min_tiles = env("KZV_NT256P_MIN_TILES", 150);
        if (nt256f_min_tiles < 0) nt256f_min_tiles = env("KZV_NT256P_MIN_TILES", 384);
        if (nt256_min_tiles < 0) nt256_min_tiles = env("KZV_NT256_MIN_TILES", 384);
        if (nt256h_min_tiles < 0) nt256h_min_tiles = env("KZV_NT256H_MIN_TILES", 768);
        if (nth_stagger < 0) nth_stagger = env("KZV_NTH_STAGGER", 8);
        if (nt_strip == -1000) {
            nt_strip = env("KZV_NT_STRIP", 3);
            if (nt_strip < 0 || nt_strip > 255) nt_strip = 0;
            if (env("KZV_BF16_DRAIN", 1) != 0) nt_strip |= 0x100;
        }
        if (rows_max_m < 0) rows_max_m = env("KZV_ROWS_MAX_M", 0);
        if (tn_schedule < 0) tn_schedule = env("KZV_TN_FREE", 1) != 0;
        if (tn256_min_tiles < 0) tn256_min_tiles = env("KZV_TN256_MIN_TILES", 9);
        if (pair < 0) pair = env("KZV_PAIR", 0) != 0;
        if (pair_r == -2) pair_r = env("KZV_PAIR_R", -1);
        if (tn_minsteps < 0) tn_minsteps = env("KZV_TN_MINSTEPS", 16);
        if (tn_blocks < 0) tn_blocks = env("KZV_TN_BLOCKS", 512);
    }
};

// What a plan needs to know about the process besides the switches.  `reserve` = kzv_cu_reserve() (host.cpp: KZV_CU_RESERVE and its setter).
struct KzvGemmEnv { int cus, reserve, rows_scope; };         // device CUs; CUs left to concurrent collectives; a KzvRowsScope is open

inline int kzv_cdiv(int a, int b) { return (a + b - 1) / b; }

// ---- gemm_nt ---------------------------------------------------------------------------------------------------------------------
// `es` = bytes per operand element: 2 = bf16 (kzv_gemm_nt), 1 = e4m3 (kzv_gemm_nt_fp8).  The shape has passed the entry's validation.
struct KzvNtShape { int M, N, K, n_valid; int64_t lda, ldb; int epilogue, es; };
struct KzvNtPlan {
    int rc; const char* err;      // KZV_OK, or the code and kzv_last_error text of the call
    int kernel, epilogue;         // KZV_GEMM_*; the call's KZV_EPI_* (the launcher's kernel instantiation)
    int grid, grid_y, block;
    int tiles, tilesN;           // output tiles of the kernel's tile shape, and tile columns
    int strip;                    // the 256x256 kernels' tile-walk argument (NT256: the NtParams field, bits 0..7 only); else 0
    int stagger;                  // NT256H
    int steps;                    // ROWS: the kernel template's 32-deep steps per wave (2, 8 or 32)
};

// The 256x256 kernels address their operands as a wave-uniform 64-bit base + a 32-bit per-lane byte offset (LDS-DMA): the A row panel of a
// tile and all valid rows of B must lie within 4 GiB of their bases.
inline bool kzv_nt_dma_offsets_fit(const KzvNtShape& a) {
    return (uint64_t)256 * (uint64_t)a.lda * a.es <= 0xffffffffull && (uint64_t)a.n_valid * (uint64_t)a.ldb * a.es <= 0xffffffffull;
}
// the persistent 256x256 K loops (256p, 256f, the pair kernel) take an even number of 64-deep K-tiles (odd: gemm_nt256.hip)
inline bool kzv_nt256p_shape_ok(const KzvNtShape& a) { return a.K >= 128 && a.K % 128 == 0 && kzv_nt_dma_offsets_fit(a); }
// free-running kernels (256f, 256h): every tile of `width` columns starts on a valid column, and a row holds a DMA piece (the clamp needs one)
inline bool kzv_nt_tiles_start_valid(const KzvNtShape& a, int tilesN, int width) {
    return a.n_valid > (tilesN - 1) * width && a.lda * 2 >= 128 && a.ldb * 2 >= 128;
}

inline KzvNtPlan kzv_nt_plan(const KzvNtShape& a, const KzvGemmSwitches& sw, const KzvGemmEnv& env) {
    KzvNtPlan pl{};
    pl.rc = KZV_OK;
    const int e = pl.epilogue = a.epilogue;
    const int tilesN = kzv_cdiv(a.N, 256), tiles = kzv_cdiv(a.M, 256) * tilesN;
    if (a.es == 1) {
        // fp8: one kernel, no fallback; KZV_NT_GRID and the CU reserve do not apply.  K >= 256, K % 256 == 0 and the four epilogues are
        // kzv_gemm_nt_fp8's validation (K > 0 and K % 256 == 0 imply K >= 256), so only the offsets can still refuse.
        if (!kzv_nt_dma_offsets_fit(a)) { pl.rc = KZV_E_ARG; pl.err = "gemm_nt_fp8: operand panel beyond the 32-bit LDS-DMA offsets"; return pl; }
        pl.kernel = KZV_GEMM_NT256P_F8; pl.tiles = tiles; pl.tilesN = tilesN;
        pl.grid = tiles < env.cus ? tiles : env.cus; pl.grid_y = 1; pl.block = 512; pl.strip = sw.nt_strip;
        return pl;
    }
    if (e < KZV_EPI_BF16 || e > KZV_EPI_GELU_F32) { pl.rc = KZV_E_ARG; pl.err = "gemm_nt: unknown epilogue"; return pl; }
    // few rows (gemm_rows.hip): inside a KzvRowsScope (the generation step) for M <= 4096, elsewhere only below rows_max_m (default 0:
    // never), so that the training step and its parity tests keep running the tiled kernels at every size
    if (a.M <= (env.rows_scope > 0 ? 4096 : sw.rows_max_m) && a.K <= 4096) {
        const int per = (a.K / 32 + 3) / 4;                               // 32-deep steps per wave
        pl.kernel = KZV_GEMM_ROWS; pl.grid = kzv_cdiv(a.N, 64); pl.grid_y = kzv_cdiv(a.M, 16); pl.block = 256;
        pl.tiles = pl.grid * pl.grid_y; pl.tilesN = pl.grid;
        pl.steps = per <= 2 ? 2 : per <= 8 ? 8 : 32;
        return pl;
    }
    // large shapes: 256x256 eight-phase kernels.  The persistent one wins wherever its per-wave drain is light (one store per element:
    // -2..-10 % vs the one-tile-per-workgroup kernel); the two-store GELU epilogues are faster through the workgroup-wide LDS epilogue
    // of gemm_nt256.hip (512-B / 1-KiB row segments).  The persistent kernels size their grid by the whole device: none with a CU reserve.
    const bool two_store = !sw.nt256p_gelu && (e == KZV_EPI_GELU || e == KZV_EPI_GELU_F32);
    pl.grid_y = 1;
    if ((sw.nt_schedule & 2) && ((sw.nt_half_mask >> e) & 1) && a.K <= sw.nth_max_k && env.reserve == 0) {
        const int tilesNh = kzv_cdiv(a.N, 128), tilesH = kzv_cdiv(a.M, 256) * tilesNh;
        // K % 384: six K-tile bodies per round of the slot / fragment-set pattern
        if (a.K >= 384 && a.K % 384 == 0 && tilesH >= sw.nt256h_min_tiles && kzv_nt_dma_offsets_fit(a) && kzv_nt_tiles_start_valid(a, tilesNh, 128)) {
            pl.kernel = KZV_GEMM_NT256H; pl.tiles = tilesH; pl.tilesN = tilesNh;
            pl.grid = tilesH < 2 * env.cus ? tilesH : 2 * env.cus; pl.block = 256;
            pl.strip = (sw.nt_strip & 0xff) * 2; pl.stagger = sw.nth_stagger;
            return pl;
        }
    }
    pl.tiles = tiles; pl.tilesN = tilesN; pl.block = 512;
    if (sw.nt256p && !two_store && env.reserve == 0 && kzv_nt256p_shape_ok(a)) {
        pl.strip = sw.nt_strip;
        pl.grid = tiles < env.cus ? tiles : env.cus;
        if ((sw.nt_schedule & 1) && tiles >= sw.nt256f_min_tiles && kzv_nt_tiles_start_valid(a, tilesN, 256)) { pl.kernel = KZV_GEMM_NT256F; return pl; }
        if (tiles >= sw.nt256p_min_tiles) {
            if (sw.nt_grid > 0 && sw.nt_grid < pl.grid) pl.grid = sw.nt_grid;
            pl.kernel = KZV_GEMM_NT256P;
            return pl;
        }
    }
    pl.strip = sw.nt_strip & 0xff;
    if (a.K >= 128 && tiles >= sw.nt256_min_tiles && kzv_nt_dma_offsets_fit(a)) { pl.kernel = KZV_GEMM_NT256; pl.grid = tiles; return pl; }
    // Measured on MI355X (tools/dev/gemm_bench.py, round 1): 128x128x64 / 2-stage ring / 2 workgroups per CU is the fastest of the
    // variants gemm.hip's template expresses, so only it is instantiated.
    pl.kernel = KZV_GEMM_NT128; pl.tilesN = kzv_cdiv(a.N, 128); pl.tiles = kzv_cdiv(a.M, 128) * pl.tilesN;
    pl.grid = pl.tiles; pl.block = 256; pl.strip = 0;
    return pl;
}

// ---- gemm_tn ---------------------------------------------------------------------------------------------------------------------
struct KzvTnShape { int Mtok, N, K, n_store; int64_t ldp, ldq, ldo; };      // has passed kzv_gemm_tn's validation
struct KzvTnPlan {
    int kernel;                   // KZV_GEMM_TN256F, TN256 (tiles of 256x256) or TN128 (tiles of 128x128)
    int tiles, splits, chunk;     // output tiles; token splits; tokens per split (a multiple of 64)
    int grid, block;
};

// gemm_tn256.hip's twin of kzv_nt_dma_offsets_fit: a 64-token stage of P and of Q within the 32-bit per-lane LDS-DMA offsets
inline bool kzv_tn_dma_offsets_fit(const KzvTnShape& a) {
    return (uint64_t)64 * (uint64_t)a.ldp * 2 + (uint64_t)a.N * 2 <= 0xffffffffull && (uint64_t)64 * (uint64_t)a.ldq * 2 + (uint64_t)a.K * 2 <= 0xffffffffull;
}
inline int kzv_tn256_tiles(const KzvTnShape& a) { return kzv_cdiv(a.N, 256) * kzv_cdiv(a.K, 256); }
// what the 256x256 weight-gradient kernels ask of a shape, the pair kernel included: enough tiles, whole 64-token stages, offsets
inline bool kzv_tn256_shape_ok(const KzvTnShape& a, const KzvGemmSwitches& sw) {
    return kzv_tn256_tiles(a) >= sw.tn256_min_tiles && a.Mtok % 64 == 0 && kzv_tn_dma_offsets_fit(a);
}

// The 128x128 kernel: token splits of one problem given the workgroup budget `target` it may fill: ONE resident round without
// overshooting it, and >= tn_minsteps reduction steps per workgroup so the 64 float atomics per lane of the epilogue (issue-bound, and
// contended when many splits hit one small output) stay a small share.
inline KzvTnPlan kzv_tn128_plan(const KzvTnShape& a, int target, const KzvGemmSwitches& sw) {
    KzvTnPlan pl{};
    pl.kernel = KZV_GEMM_TN128; pl.block = 256;
    pl.tiles = kzv_cdiv(a.N, 128) * kzv_cdiv(a.K, 128);
    const int tok_tiles = kzv_cdiv(a.Mtok, 64);
    int splits = target / pl.tiles;
    if (splits > tok_tiles / sw.tn_minsteps) splits = tok_tiles / sw.tn_minsteps;
    if (splits > tok_tiles) splits = tok_tiles;
    if (splits < 1) splits = 1;
    const int chunk_tiles = kzv_cdiv(tok_tiles, splits);
    pl.splits = kzv_cdiv(tok_tiles, chunk_tiles); pl.chunk = chunk_tiles * 64;
    pl.grid = pl.tiles * pl.splits;
    return pl;
}

// One decision cannot be made ahead: a TN256* plan needs a partial-tile workspace, and when none can be had the launch falls back to
// kzv_tn128_plan(a, sw.tn_blocks, sw) (kzv_gemm_tn).
inline KzvTnPlan kzv_tn_plan(const KzvTnShape& a, const KzvGemmSwitches& sw, const KzvGemmEnv& env) {
    const int tok_tiles = a.Mtok / 64;
    // (the kernel also needs N >= 8, K >= 8, K % 4 == 0, ldo % 4 == 0 and a 16-byte aligned OUT; no check here: kzv_tn_validate has
    // N > 0, K > 0, N % 8 == 0, K % 8 == 0, ldo % 4 == 0 and the alignment in front of every plan)
    if (kzv_tn256_shape_ok(a, sw) && tok_tiles >= 2) {
        KzvTnPlan pl{};
        pl.tiles = kzv_tn256_tiles(a);
        // one workgroup per CU in total, the reserved CUs left to a concurrent collective; every split keeps >= 8 reduction stages
        // (and at least 2: the prologue stages two)
        int cus = env.cus - env.reserve;
        if (sw.tn_cus > 0 && sw.tn_cus < cus) cus = sw.tn_cus;
        int splits = cus / pl.tiles;
        if (splits > tok_tiles / 8) splits = tok_tiles / 8;
        if (splits < 1) splits = 1;
        int chunk_tiles = kzv_cdiv(tok_tiles, splits);
        if (chunk_tiles < 2) chunk_tiles = 2;
        splits = kzv_cdiv(tok_tiles, chunk_tiles);
        if (tok_tiles - (splits - 1) * chunk_tiles >= 2) {              // (a one-stage last split: the 128x128 kernel)
            pl.kernel = sw.tn_schedule ? KZV_GEMM_TN256F : KZV_GEMM_TN256;
            pl.splits = splits; pl.chunk = chunk_tiles * 64;
            pl.grid = pl.tiles * splits; pl.block = 512;
            return pl;
        }
    }
    return kzv_tn128_plan(a, sw.tn_blocks, sw);
}

// Grouped launch of the 128x128 kernel (kzv_gemm_tn_group): n independent weight gradients in one grid.  A problem of 24 or more
// 256x256 tiles of n_store x K is launched on its own (kzv_gemm_tn).  The 24 is round 2's threshold of the 256x256 kernel and OLDER
// than tn256_min_tiles = 9: it is kept on purpose -- between 9 and 23 tiles a grouped problem stays in the group although alone it would take
// the 256x256 kernel.  Changing it is a measured lead for DESIGN section 8, not a clean-up.
constexpr int KZV_TN_GROUP_OWN_TILES = 24;
constexpr int KZV_TN_GROUP_MAX = 40;     // 88-byte descriptors in the kernel arguments (4 KiB): the 36 weight gradients of a six-layer decoder in one grid
inline bool kzv_tn_group_own_launch(const KzvTnShape& a) { return kzv_cdiv(a.n_store, 256) * kzv_cdiv(a.K, 256) >= KZV_TN_GROUP_OWN_TILES; }
struct KzvTnGroupPlan { int n; int splits[KZV_TN_GROUP_MAX], chunk[KZV_TN_GROUP_MAX], start[KZV_TN_GROUP_MAX + 1]; int grid; };
// a[0..n): the grouped problems (none of them kzv_tn_group_own_launch), 1 <= n <= KZV_TN_GROUP_MAX.  The workgroup budget is shared in
// proportion to the tile counts.
inline KzvTnGroupPlan kzv_tn_group_plan(const KzvTnShape* a, int n, const KzvGemmSwitches& sw) {
    KzvTnGroupPlan g{};
    g.n = n;
    int tiles_total = 0;
    for (int i = 0; i < n; ++i) tiles_total += kzv_cdiv(a[i].N, 128) * kzv_cdiv(a[i].K, 128);
    // one resident round (512 workgroups) for the small groups; a group with more tiles than that round's half (the 36 weight
    // gradients of the decoder's layers: 288 tiles) takes two: 3 token splits of 80 stages, 261 us against 335 with one split per
    // tile and 348 for six launches of ten splits (tools/dev/r5_tnblocks.sh)
    const int target = tiles_total >= 256 ? 2 * sw.tn_blocks : sw.tn_blocks;
    int blocks = 0;
    for (int i = 0; i < n; ++i) {
        const int tiles = kzv_cdiv(a[i].N, 128) * kzv_cdiv(a[i].K, 128);
        int share = (int)((int64_t)target * tiles / tiles_total);
        if (share < tiles) share = tiles;
        const KzvTnPlan pl = kzv_tn128_plan(a[i], share, sw);
        g.splits[i] = pl.splits; g.chunk[i] = pl.chunk; g.start[i] = blocks;
        blocks += pl.grid;
    }
    g.start[n] = g.grid = blocks;
    return g;
}

// ---- the dgrad + wgrad pair launch (gemm_tn256.hip) ----------------------------------------------------------------------------------
// Every workgroup runs its gemm_nt tiles and then ONE token range of ONE weight-gradient tile, sized so that all finish together.
struct KzvPairTable { unsigned short tile[256], split[256], t0[256], cnt[256]; };      // by blockIdx; cnt == 0: no weight-gradient share
struct KzvPairPlan { int grid, tiles, tilesN, strip, per, tilesKw, splits; KzvPairTable table; };

// what can be said before looking at the shapes: the switch, no CU reserve, the free-running weight-gradient schedule, a 256-CU
// device (the table is by workgroup), a one-store epilogue
inline bool kzv_pair_enabled(int epilogue, const KzvGemmSwitches& sw, const KzvGemmEnv& env) {
    if (!sw.pair || env.reserve != 0 || !sw.tn_schedule || env.cus != 256) return false;
    return epilogue == KZV_EPI_BF16 || epilogue == KZV_EPI_F32 || epilogue == KZV_EPI_DGELU || epilogue == KZV_EPI_RESID;
}
// stages of the weight-gradient loop one gemm_nt tile is worth: (K-tiles x 1.45 us + drain) / 1.55 us per stage; KZV_PAIR_R overrides (x 0.01)
inline double kzv_pair_ratio(int nk, int epilogue, const KzvGemmSwitches& sw) {
    const double drain = (epilogue == KZV_EPI_DGELU || epilogue == KZV_EPI_RESID) ? 5.0 : 2.5;
    const double r = 0.6 * (nk * 1.45 + drain) / 1.55;          // 0.6: the best of a sweep over 0 / 0.6 / 1 / 1.4 / 2 (flat between 0 and 0.6)
    return sw.pair_r >= 0 ? r * sw.pair_r * 0.01 / 0.6 : r;
}
// The two halves of the pair's conditions (each shape has passed its entry's validation): the persistent kernel's and the 256x256
// weight-gradient kernel's own, with stricter bounds -- >= 256 gemm_nt tiles whatever nt256p_min_tiles says, <= 128 weight-gradient
// tiles, >= 8 stages per split.  Both hold: the pair is launched (the levelling below never refuses; tests/host/gemm_plan_main.cpp).
inline bool kzv_pair_nt_ok(const KzvNtShape& na, const KzvGemmSwitches& sw, const KzvGemmEnv& env) {
    return kzv_pair_enabled(na.epilogue, sw, env) && kzv_nt256p_shape_ok(na) && kzv_cdiv(na.M, 256) * kzv_cdiv(na.N, 256) >= 256;
}
inline bool kzv_pair_tn_ok(const KzvTnShape& ta, const KzvGemmSwitches& sw) {
    const int per = kzv_tn256_tiles(ta), stages = ta.Mtok / 64;
    if (!kzv_tn256_shape_ok(ta, sw) || per > 128) return false;
    const int S = 256 / per;
    return S >= 1 && stages >= 8 * S && stages <= 65000;
}
inline bool kzv_pair_plan(const KzvNtShape& na, const KzvTnShape& ta, const KzvGemmSwitches& sw, const KzvGemmEnv& env, KzvPairPlan* out) {
    if (!kzv_pair_nt_ok(na, sw, env) || !kzv_pair_tn_ok(ta, sw)) return false;
    const int tilesN = kzv_cdiv(na.N, 256), tiles = kzv_cdiv(na.M, 256) * tilesN;
    const int tilesKw = kzv_cdiv(ta.K, 256), tilesNw = kzv_cdiv(ta.N, 256), per = tilesNw * tilesKw;
    const int stages = ta.Mtok / 64;
    const int G = 256, S = G / per;
    KzvPairTable& plan = out->table;
    int cb[256], idb[256];
    const int nwg = per * S;
    for (int b = 0; b < G; ++b) {
        const int vblk = (b & 7) * (G >> 3) + (b >> 3);
        cb[b] = vblk < tiles ? (tiles - 1 - vblk) / G + 1 : 0;
        idb[b] = -1;
        plan.tile[b] = plan.split[b] = plan.t0[b] = plan.cnt[b] = 0;
        if (b < nwg) {
            const int xcd = b & 7, q = nwg >> 3, r = nwg & 7;                      // kzv_common.h xcd_remap
            idb[b] = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (b >> 3);
        }
    }
    const double r = kzv_pair_ratio(na.K / 64, na.epilogue, sw);
    std::vector<int> cg((size_t)tilesNw * S, 0);                                    // gemm_nt tiles of the group (tile row, split): the largest of its members
    for (int b = 0; b < nwg; ++b) { const int sp = idb[b] / per, tl = idb[b] % per; int& c = cg[(size_t)(tl / tilesKw) * S + sp]; c = cb[b] > c ? cb[b] : c; }
    std::vector<int> t0((size_t)tilesNw * S), cnt((size_t)tilesNw * S);
    for (int tn = 0; tn < tilesNw; ++tn) {
        double csum = 0;
        for (int sp = 0; sp < S; ++sp) csum += cg[(size_t)tn * S + sp];
        const double level = (stages + r * csum) / S;                               // the common finishing time, in stages
        double acc = 0; int prev = 0;
        for (int sp = 0; sp < S; ++sp) {
            double n = level - r * cg[(size_t)tn * S + sp];
            if (n < 2) n = 2;
            acc += n;
            int end = sp == S - 1 ? stages : (int)(acc + 0.5);
            const int left = S - 1 - sp;                                             // every later split keeps >= 2 stages
            if (end > stages - 2 * left) end = stages - 2 * left;
            if (end < prev + 2) end = prev + 2;
            t0[(size_t)tn * S + sp] = prev; cnt[(size_t)tn * S + sp] = end - prev; prev = end;
        }
        if (prev != stages) return false;
    }
    for (int b = 0; b < nwg; ++b) {
        const int sp = idb[b] / per, tl = idb[b] % per; const size_t gi = (size_t)(tl / tilesKw) * S + sp;
        plan.tile[b] = (unsigned short)tl; plan.split[b] = (unsigned short)sp; plan.t0[b] = (unsigned short)t0[gi]; plan.cnt[b] = (unsigned short)cnt[gi];
    }
    out->grid = G; out->tiles = tiles; out->tilesN = tilesN; out->strip = sw.nt_strip;
    out->per = per; out->tilesKw = tilesKw; out->splits = S;
    return true;
}

#pragma GCC visibility pop
