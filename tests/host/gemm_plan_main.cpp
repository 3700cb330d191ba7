// Drives csrc/gemm_plan.h (no HIP, no GPU).  tests/test_gemm_plan_cpu.py builds it with -fsanitize=address,undefined and runs it: a check
// that fails prints its line and exits 1.
//   Part 1: the dispatch as it was BEFORE the planner -- the chain of "did you take it?" launchers of kzv_gemm_nt / kzv_gemm_tn /
//           kzv_gemm_tn_group / kzv_gemm_pair_launch, transcribed gate by gate in their order (each launcher re-deriving its tile counts, as
//           it did), with the launch it would have made recorded instead of made -- and planner == transcription on every field over a
//           sweep of shapes, epilogues, switches and environments.  This is the record of what the chain was.
//   Part 2: named expectations for the benchmark's shapes at 256 CUs and default switches.
//   Part 3: invariants of the token splits, the pair table and the group plan over the swept shapes.
#include "../../kuzushiji-vision_amd/csrc/gemm_plan.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>

#define CHECK(cond) do { if (!(cond)) { std::fprintf(stderr, "%s:%d: CHECK failed: %s\n   %s\n", __FILE__, __LINE__, #cond, g_ctx); std::exit(1); } } while (0)

namespace {

char g_ctx[512] = "";

// ---- a fake environment: the defaults, or the variables the caller sets --------------------------------------------------------------
struct Var { const char* name; int value; };
const Var* g_vars = nullptr; int g_nvars = 0;
int fake_env(const char* name, int dflt) {
    for (int i = 0; i < g_nvars; ++i) if (!std::strcmp(g_vars[i].name, name)) return g_vars[i].value;
    return dflt;
}
KzvGemmSwitches switches(const Var* vars = nullptr, int n = 0) {
    g_vars = vars; g_nvars = n;
    KzvGemmSwitches sw;
    sw.resolve(fake_env);
    return sw;
}

// ======================================================================================================================================
// Part 1: the chain before the planner.  `p` stands for the NtParams / TnParams the launchers were given; a switch that was a lazily
// read static is the KzvGemmSwitches field of the same variable.
// ======================================================================================================================================
struct OldNt { int M, N, K, n_valid; int64_t lda, ldb; };
struct Launch { int kernel, grid, grid_y, block, tiles, tilesN, strip, stagger, steps; };

bool old_nt_dma_offsets_fit(const OldNt& p, int es) {
    return (uint64_t)256 * (uint64_t)p.lda * es <= 0xffffffffull && (uint64_t)p.n_valid * (uint64_t)p.ldb * es <= 0xffffffffull;
}
bool known(int epilogue) { return epilogue >= 0 && epilogue <= 5; }      // the launchers' `default: return 0`

int old_rows_launch(const OldNt& p, int epilogue, const KzvGemmSwitches& sw, const KzvGemmEnv& env, Launch* l) {
    if (p.M > (env.rows_scope > 0 ? 4096 : sw.rows_max_m)) return 0;
    if (p.K > 4096) return 0;
    const int per = (p.K / 32 + 3) / 4;
    if (!known(epilogue)) return 0;
    *l = Launch{KZV_GEMM_ROWS, (p.N + 63) / 64, (p.M + 15) / 16, 256, ((p.N + 63) / 64) * ((p.M + 15) / 16), (p.N + 63) / 64, 0, 0,
                per <= 2 ? 2 : per <= 8 ? 8 : 32};
    return 1;
}
int old_nt256h_launch(const OldNt& p, int epilogue, const KzvGemmSwitches& sw, const KzvGemmEnv& env, Launch* l) {
    const int tilesN = (p.N + 127) / 128;
    const int tiles = ((p.M + 255) / 256) * tilesN;
    if (p.K < 384 || p.K % 384 || tiles < sw.nt256h_min_tiles) return 0;
    if (!old_nt_dma_offsets_fit(p, 2)) return 0;
    if (p.n_valid <= (tilesN - 1) * 128 || p.lda * 2 < 128 || p.ldb * 2 < 128) return 0;
    const int grid = tiles < 2 * env.cus ? tiles : 2 * env.cus;
    const int strip = (sw.nt_strip & 0xff) * 2;
    if (!known(epilogue)) return 0;
    *l = Launch{KZV_GEMM_NT256H, grid, 1, 256, tiles, tilesN, strip, sw.nth_stagger, 0};
    return 1;
}
int old_nt256f_launch(const OldNt& p, int epilogue, const KzvGemmSwitches& sw, const KzvGemmEnv& env, Launch* l) {
    const int tilesN = (p.N + 255) / 256;
    const int tiles = ((p.M + 255) / 256) * tilesN;
    if (p.K < 128 || p.K % 128 || tiles < sw.nt256f_min_tiles) return 0;
    if (!old_nt_dma_offsets_fit(p, 2)) return 0;
    if (p.n_valid <= (tilesN - 1) * 256 || p.lda * 2 < 128 || p.ldb * 2 < 128) return 0;
    const int grid = tiles < env.cus ? tiles : env.cus;
    if (!known(epilogue)) return 0;
    *l = Launch{KZV_GEMM_NT256F, grid, 1, 512, tiles, tilesN, sw.nt_strip, 0, 0};
    return 1;
}
int old_nt256p_launch(const OldNt& p, int epilogue, const KzvGemmSwitches& sw, const KzvGemmEnv& env, Launch* l) {
    const int tilesN = (p.N + 255) / 256;
    const int tiles = ((p.M + 255) / 256) * tilesN;
    if (p.K < 128 || p.K % 128 || tiles < sw.nt256p_min_tiles) return 0;
    if (!old_nt_dma_offsets_fit(p, 2)) return 0;
    int grid = tiles < env.cus ? tiles : env.cus;
    { const int g = sw.nt_grid; if (g > 0 && g < grid) grid = g; }
    if (!known(epilogue)) return 0;
    *l = Launch{KZV_GEMM_NT256P, grid, 1, 512, tiles, tilesN, sw.nt_strip, 0, 0};
    return 1;
}
int old_nt256_launch(const OldNt& p, int epilogue, const KzvGemmSwitches& sw, const KzvGemmEnv&, Launch* l) {
    const int tiles = ((p.M + 255) / 256) * ((p.N + 255) / 256);
    if (p.K < 128 || tiles < sw.nt256_min_tiles) return 0;
    if (!old_nt_dma_offsets_fit(p, 2)) return 0;
    if (!known(epilogue)) return 0;
    *l = Launch{KZV_GEMM_NT256, tiles, 1, 512, tiles, (p.N + 255) / 256, sw.nt_strip & 0xff, 0, 0};      // (the kernel walks by p.strip)
    return 1;
}
// kzv_gemm_nt after its validation: 0 and *l, or the error code
int old_gemm_nt(const OldNt& p, int epilogue, const KzvGemmSwitches& sw, const KzvGemmEnv& env, Launch* l, const char** err) {
    const int use_p = sw.nt256p;
    if (old_rows_launch(p, epilogue, sw, env, l)) return 0;
    const int p_gelu = sw.nt256p_gelu;
    const bool two_store = !p_gelu && (epilogue == KZV_EPI_GELU || epilogue == KZV_EPI_GELU_F32);
    const int half_maxk = sw.nth_max_k;
    if ((sw.nt_schedule & 2) && known(epilogue) && ((sw.nt_half_mask >> epilogue) & 1) && p.K <= half_maxk && env.reserve == 0 && old_nt256h_launch(p, epilogue, sw, env, l)) return 0;
    if ((sw.nt_schedule & 1) && use_p && !two_store && env.reserve == 0 && old_nt256f_launch(p, epilogue, sw, env, l)) return 0;
    if (use_p && !two_store && env.reserve == 0 && old_nt256p_launch(p, epilogue, sw, env, l)) return 0;
    if (old_nt256_launch(p, epilogue, sw, env, l)) return 0;
    if (!known(epilogue)) { *err = "gemm_nt: unknown epilogue"; return KZV_E_ARG; }
    const int grid = ((p.M + 2 * 64 - 1) / (2 * 64)) * ((p.N + 2 * 64 - 1) / (2 * 64));
    *l = Launch{KZV_GEMM_NT128, grid, 1, 2 * 2 * 64, grid, (p.N + 127) / 128, 0, 0, 0};
    return 0;
}
int old_nt256p_fp8_launch(const OldNt& p, int epilogue, const KzvGemmSwitches& sw, const KzvGemmEnv& env, Launch* l, const char** err) {
    const int tilesN = (p.N + 255) / 256;
    const int tiles = ((p.M + 255) / 256) * tilesN;
    if (p.K < 256 || p.K % 256) { *err = "gemm_nt_fp8: K must be a multiple of 256 (an even number of 128-byte K-tiles)"; return KZV_E_ARG; }
    if (!old_nt_dma_offsets_fit(p, 1)) { *err = "gemm_nt_fp8: operand panel beyond the 32-bit LDS-DMA offsets"; return KZV_E_ARG; }
    const int grid = tiles < env.cus ? tiles : env.cus;
    if (epilogue != KZV_EPI_BF16 && epilogue != KZV_EPI_GELU && epilogue != KZV_EPI_RESID && epilogue != KZV_EPI_DGELU) { *err = "gemm_nt_fp8: epilogue must be BF16, GELU, RESID or DGELU"; return KZV_E_ARG; }
    *l = Launch{KZV_GEMM_NT256P_F8, grid, 1, 512, tiles, tilesN, sw.nt_strip, 0, 0};
    return 0;
}

struct OldTn { int Mtok, N, K, n_store, splits, chunk; int64_t ldp, ldq, ldo; };
bool old_tn_dma_offsets_fit(const OldTn& p) {
    return (uint64_t)64 * (uint64_t)p.ldp * 2 + (uint64_t)p.N * 2 <= 0xffffffffull && (uint64_t)64 * (uint64_t)p.ldq * 2 + (uint64_t)p.K * 2 <= 0xffffffffull;
}
int old_tn_plan(OldTn& p, int target, const KzvGemmSwitches& sw) {
    const int min_steps = sw.tn_minsteps;
    const int tiles = ((p.N + 127) / 128) * ((p.K + 127) / 128);
    const int tok_tiles = (p.Mtok + 63) / 64;
    int splits = target / tiles;
    if (splits > tok_tiles / min_steps) splits = tok_tiles / min_steps;
    if (splits > tok_tiles) splits = tok_tiles;
    if (splits < 1) splits = 1;
    const int chunk_tiles = (tok_tiles + splits - 1) / splits;
    splits = (tok_tiles + chunk_tiles - 1) / chunk_tiles;
    p.splits = splits; p.chunk = chunk_tiles * 64;
    return tiles * splits;
}
// kzv_tn256_launch up to the workspace claim (OUT is 16-byte aligned: kzv_tn_params)
int old_tn256_launch(const OldTn& p0, const KzvGemmSwitches& sw, const KzvGemmEnv& env, KzvTnPlan* l) {
    const int tiles = ((p0.N + 255) / 256) * ((p0.K + 255) / 256);
    const int tok_tiles = p0.Mtok / 64;
    if (tiles < sw.tn256_min_tiles || p0.Mtok % 64 || tok_tiles < 2 || p0.N < 8 || p0.K < 8) return 0;
    if (!old_tn_dma_offsets_fit(p0)) return 0;
    OldTn p = p0;
    int cus = env.cus - env.reserve;
    { const int g = sw.tn_cus; if (g > 0 && g < cus) cus = g; }
    int splits = cus / tiles;
    if (splits > tok_tiles / 8) splits = tok_tiles / 8;
    if (splits < 1) splits = 1;
    int chunk_tiles = (tok_tiles + splits - 1) / splits;
    if (chunk_tiles < 2) chunk_tiles = 2;
    splits = (tok_tiles + chunk_tiles - 1) / chunk_tiles;
    if (tok_tiles - (splits - 1) * chunk_tiles < 2) return 0;
    p.splits = splits; p.chunk = chunk_tiles * 64;
    if (p.K % 4 || p.ldo % 4) return 0;
    *l = KzvTnPlan{sw.tn_schedule ? KZV_GEMM_TN256F : KZV_GEMM_TN256, tiles, p.splits, p.chunk, tiles * splits, 512};
    return 1;
}
KzvTnPlan old_gemm_tn(const OldTn& p0, const KzvGemmSwitches& sw, const KzvGemmEnv& env) {
    KzvTnPlan l{};
    if (old_tn256_launch(p0, sw, env, &l)) return l;
    OldTn p = p0;
    const int blocks = old_tn_plan(p, sw.tn_blocks, sw);
    return KzvTnPlan{KZV_GEMM_TN128, ((p.N + 127) / 128) * ((p.K + 127) / 128), p.splits, p.chunk, blocks, 256};
}
// kzv_gemm_tn_group, 2 <= n <= 40: own[i] = launched on its own; the grouped ones' splits / chunk / start in their order
struct OldGroup { int n; bool own[40]; int splits[40], chunk[40], start[41]; };
OldGroup old_gemm_tn_group(const OldTn* a, int n, const KzvGemmSwitches& sw) {
    OldGroup g{};
    OldTn gp[40];
    int tiles_total = 0;
    for (int i = 0; i < n; ++i) {
        const OldTn& p = a[i];
        const int t256 = ((p.n_store + 255) / 256) * ((p.K + 255) / 256);
        if (t256 >= 24) { g.own[i] = true; continue; }
        gp[g.n++] = p;
        tiles_total += ((p.N + 127) / 128) * ((p.K + 127) / 128);
    }
    int blocks = 0;
    for (int i = 0; i < g.n; ++i) {
        const int tiles = ((gp[i].N + 127) / 128) * ((gp[i].K + 127) / 128);
        const int target = tiles_total >= 256 ? 2 * sw.tn_blocks : sw.tn_blocks;
        int share = (int)((int64_t)target * tiles / tiles_total);
        if (share < tiles) share = tiles;
        g.start[i] = blocks;
        blocks += old_tn_plan(gp[i], share, sw);
        g.splits[i] = gp[i].splits; g.chunk[i] = gp[i].chunk;
    }
    g.start[g.n] = blocks;
    return g;
}
// kzv_gemm_pair_launch down to "the plan": would it have gone on to build one?
bool old_pair_gate(const OldNt& pn, int epilogue, const OldTn& pt, const KzvGemmSwitches& sw, const KzvGemmEnv& env) {
    if (!sw.pair || env.reserve != 0 || !sw.tn_schedule || env.cus != 256) return false;
    if (epilogue != KZV_EPI_BF16 && epilogue != KZV_EPI_F32 && epilogue != KZV_EPI_DGELU && epilogue != KZV_EPI_RESID) return false;
    const int tilesN = (pn.N + 255) / 256, tiles = ((pn.M + 255) / 256) * tilesN;
    if (pn.K < 128 || pn.K % 128 || tiles < 256) return false;
    if (!old_nt_dma_offsets_fit(pn, 2)) return false;
    const int tilesKw = (pt.K + 255) / 256, tilesNw = (pt.N + 255) / 256, per = tilesNw * tilesKw;
    const int stages = pt.Mtok / 64;
    if (per < sw.tn256_min_tiles || per > 128 || pt.Mtok % 64) return false;
    if (!old_tn_dma_offsets_fit(pt)) return false;
    const int G = 256, S = G / per;
    if (S < 1 || stages < 8 * S || stages > 65000) return false;
    return true;
}

// ======================================================================================================================================
const int EPIS[] = {KZV_EPI_BF16, KZV_EPI_F32, KZV_EPI_GELU, KZV_EPI_RESID, KZV_EPI_DGELU, KZV_EPI_GELU_F32};
const Var MIN1[] = {{"KZV_NT256P_MIN_TILES", 1}, {"KZV_NT256_MIN_TILES", 1}};      // test_reference_fixtures_through_the_256x256_gemm_kernels
const Var TN_MIN1[] = {{"KZV_TN256_MIN_TILES", 1}, {"KZV_TN_MINSTEPS", 4}, {"KZV_TN_BLOCKS", 300}};

void same_nt(const KzvNtPlan& pl, int rc, const char* err, const Launch& l) {
    CHECK(pl.rc == rc);
    if (rc != KZV_OK) { CHECK(pl.err && !std::strcmp(pl.err, err)); return; }
    CHECK(pl.kernel == l.kernel); CHECK(pl.grid == l.grid); CHECK(pl.grid_y == l.grid_y); CHECK(pl.block == l.block);
    CHECK(pl.tiles == l.tiles); CHECK(pl.tilesN == l.tilesN); CHECK(pl.strip == l.strip); CHECK(pl.stagger == l.stagger); CHECK(pl.steps == l.steps);
}

long sweep_nt() {
    const int Ms[] = {1, 64, 1024, 4097, 24600, 33024, 41216}, Ns[] = {64, 256, 768, 1024, 2304, 3072, 4352}, Ks[] = {64, 128, 320, 384, 768, 1536, 3072};
    long plans = 0, by_kernel[7] = {0, 0, 0, 0, 0, 0, 0};
    for (int setting = 0; setting < 4; ++setting) {
        // 0: defaults; 1: the two MIN_TILES = 1; 2, 3: other values than the defaults where the sweep would otherwise never leave them
        const Var other[] = {{"KZV_NT256P_GELU", 1}, {"KZV_NTH_MAX_K", 768}, {"KZV_NT_HALF_EPIS", 0x15}, {"KZV_NT_STRIP", 300}, {"KZV_BF16_DRAIN", 0}, {"KZV_NTH_STAGGER", 3},
                             {"KZV_NT256H_MIN_TILES", 100}, {"KZV_ROWS_MAX_M", 1024}};
        const Var nop[] = {{"KZV_NT256P", 0}, {"KZV_NT_STRIP", 5}};
        KzvGemmSwitches base = setting == 0 ? switches() : setting == 1 ? switches(MIN1, 2) : setting == 2 ? switches(other, 8) : switches(nop, 2);
        for (int sched = 0; sched < 4; ++sched) for (int nt_grid = 0; nt_grid <= 128; nt_grid += 128) {
            KzvGemmSwitches sw = base;
            sw.nt_schedule = sched; sw.nt_grid = nt_grid;
            for (int reserve = 0; reserve <= 32; reserve += 32) for (int scope = 0; scope < 2; ++scope) for (int cus = 256; cus >= 64; cus -= 192) {
                const KzvGemmEnv env{cus, reserve, scope};
                for (int M : Ms) for (int N : Ns) for (int K : Ks) for (int cut = 0; cut <= 24; cut += 24) for (int ei = -1; ei < 7; ++ei) {
                    const int e = ei < 0 ? -1 : ei;                       // -1 and 6: outside the six
                    const OldNt p{M, N, K, N - cut, K, K};
                    std::snprintf(g_ctx, sizeof g_ctx, "nt M=%d N=%d K=%d n_valid=%d epi=%d sched=%d nt_grid=%d reserve=%d scope=%d cus=%d setting=%d", M, N, K, N - cut, e, sched, nt_grid, reserve, scope, cus, setting);
                    Launch l{}; const char* err = "";
                    const int rc = old_gemm_nt(p, e, sw, env, &l, &err);
                    const KzvNtPlan pl = kzv_nt_plan(KzvNtShape{M, N, K, N - cut, K, K, e, 2}, sw, env);
                    same_nt(pl, rc, err, l);
                    if (rc == KZV_OK) ++by_kernel[pl.kernel];
                    ++plans;
                    if (K % 256 == 0 && (e == KZV_EPI_BF16 || e == KZV_EPI_GELU || e == KZV_EPI_RESID || e == KZV_EPI_DGELU) && sched == 0) {      // kzv_gemm_nt_fp8's validation
                        Launch l8{}; const char* err8 = "";
                        const int rc8 = old_nt256p_fp8_launch(p, e, sw, env, &l8, &err8);
                        same_nt(kzv_nt_plan(KzvNtShape{M, N, K, N - cut, K, K, e, 1}, sw, env), rc8, err8, l8);
                        ++plans;
                    }
                }
            }
        }
    }
    for (int k = KZV_GEMM_ROWS; k <= KZV_GEMM_NT128; ++k) CHECK(by_kernel[k] > 0);      // the sweep reaches every kernel
    // operand panels beyond the 32-bit LDS-DMA offsets: the 256x256 kernels decline, the fp8 entry errors
    {
        const KzvGemmSwitches sw = switches(); const KzvGemmEnv env{256, 0, 0};
        const int64_t lds[] = {1 << 22, 1 << 23, 1 << 24};
        for (int64_t ld : lds) for (int e : EPIS) {
            const OldNt p{41216, 3072, 768, 3072, ld, ld};
            std::snprintf(g_ctx, sizeof g_ctx, "nt wide ld=%lld epi=%d", (long long)ld, e);
            Launch l{}; const char* err = "";
            const int rc = old_gemm_nt(p, e, sw, env, &l, &err);
            same_nt(kzv_nt_plan(KzvNtShape{p.M, p.N, p.K, p.n_valid, ld, ld, e, 2}, sw, env), rc, err, l);
            if (e == KZV_EPI_BF16) {
                const int rc8 = old_nt256p_fp8_launch(p, e, sw, env, &l, &err);
                same_nt(kzv_nt_plan(KzvNtShape{p.M, p.N, p.K, p.n_valid, ld, ld, e, 1}, sw, env), rc8, err, l);
            }
            plans += 2;
        }
    }
    return plans;
}

// Part 3 for one tn plan: the splits cover the token tiles exactly once; a 256x256 split has >= 2 stages
void tn_invariants(const KzvTnPlan& pl, int Mtok) {
    const int tok_tiles = (Mtok + 63) / 64, chunk_tiles = pl.chunk / 64;
    CHECK(pl.chunk % 64 == 0 && pl.splits >= 1 && chunk_tiles >= 1);
    CHECK((pl.splits - 1) * chunk_tiles < tok_tiles && pl.splits * chunk_tiles >= tok_tiles);      // every split starts inside, the last one ends it
    CHECK(pl.grid == pl.tiles * pl.splits);
    if (pl.kernel != KZV_GEMM_TN128) { CHECK(chunk_tiles >= 2); CHECK(tok_tiles - (pl.splits - 1) * chunk_tiles >= 2); CHECK(Mtok % 64 == 0); }
}

long sweep_tn() {
    const int Ms[] = {41, 64, 128, 200, 1000, 4096, 4160, 8192, 33024, 41216}, Ns[] = {64, 256, 768, 1288, 1536, 2304, 3072, 4352}, Ks[] = {64, 256, 384, 768, 1024, 1280, 3072};
    long plans = 0, by_kernel[3] = {0, 0, 0};
    for (int setting = 0; setting < 2; ++setting) for (int sched = 0; sched < 2; ++sched) for (int tn_cus = 0; tn_cus <= 100; tn_cus += 100) {
        KzvGemmSwitches sw = setting ? switches(TN_MIN1, 3) : switches();
        sw.tn_schedule = sched; sw.tn_cus = tn_cus;
        for (int reserve = 0; reserve <= 32; reserve += 32) for (int cus = 256; cus >= 64; cus -= 192) {
            const KzvGemmEnv env{cus, reserve, 0};
            for (int M : Ms) for (int N : Ns) for (int K : Ks) for (int cut = 0; cut <= 8; cut += 8) {
                std::snprintf(g_ctx, sizeof g_ctx, "tn Mtok=%d N=%d K=%d n_store=%d sched=%d tn_cus=%d reserve=%d cus=%d setting=%d", M, N, K, N - cut, sched, tn_cus, reserve, cus, setting);
                const OldTn p{M, N, K, N - cut, 0, 0, N, K, K};
                const KzvTnPlan want = old_gemm_tn(p, sw, env);
                const KzvTnPlan pl = kzv_tn_plan(KzvTnShape{M, N, K, N - cut, N, K, K}, sw, env);
                CHECK(pl.kernel == want.kernel); CHECK(pl.tiles == want.tiles); CHECK(pl.splits == want.splits); CHECK(pl.chunk == want.chunk);
                CHECK(pl.grid == want.grid); CHECK(pl.block == want.block);
                tn_invariants(pl, M);
                // the launch-time fallback (no workspace) is the 128x128 plan the chain fell through to
                OldTn q = p;
                const int blocks = old_tn_plan(q, sw.tn_blocks, sw);
                const KzvTnPlan fb = kzv_tn128_plan(KzvTnShape{M, N, K, N - cut, N, K, K}, sw.tn_blocks, sw);
                CHECK(fb.kernel == KZV_GEMM_TN128 && fb.grid == blocks && fb.splits == q.splits && fb.chunk == q.chunk && fb.block == 256);
                tn_invariants(fb, M);
                ++by_kernel[pl.kernel - KZV_GEMM_TN256F];
                ++plans;
            }
        }
    }
    CHECK(by_kernel[0] > 0 && by_kernel[1] > 0 && by_kernel[2] > 0);
    {   // a stage of P beyond the 32-bit offsets: the 128x128 kernel
        const KzvGemmSwitches sw = switches(); const KzvGemmEnv env{256, 0, 0};
        std::snprintf(g_ctx, sizeof g_ctx, "tn wide ldp");
        const OldTn p{4096, 2304, 768, 2304, 0, 0, (int64_t)1 << 25, 768, 768};
        const KzvTnPlan want = old_gemm_tn(p, sw, env), pl = kzv_tn_plan(KzvTnShape{4096, 2304, 768, 2304, (int64_t)1 << 25, 768, 768}, sw, env);
        CHECK(want.kernel == KZV_GEMM_TN128 && pl.kernel == KZV_GEMM_TN128 && pl.grid == want.grid && pl.splits == want.splits && pl.chunk == want.chunk);
        ++plans;
    }
    return plans;
}

long sweep_group() {
    // the decoder's layers (hidden 256, ffn 1024, vocabulary head), an encoder layer's four, and mixtures around the 24-tile rule
    const int shapes[][2] = {{256, 256}, {1024, 256}, {256, 1024}, {768, 256}, {512, 256}, {4352, 256}, {768, 768}, {2304, 768}, {3072, 768}, {768, 3072}, {1536, 1024}, {1288, 1280}, {6144, 256}};
    const int NS = sizeof shapes / sizeof shapes[0];
    long plans = 0; int seen_own = 0, seen_kept_9_to_23 = 0;
    const KzvGemmSwitches sws[] = {switches(), switches(TN_MIN1, 3)};
    for (const KzvGemmSwitches& sw : sws) for (int Mtok : {200, 3328, 5120, 41216}) for (int n = 2; n <= 40; ++n) for (int rot = 0; rot < NS; ++rot) {
        std::snprintf(g_ctx, sizeof g_ctx, "group Mtok=%d n=%d rot=%d", Mtok, n, rot);
        OldTn a[40]; KzvTnShape sh[40]; int m = 0; bool own[40];
        for (int i = 0; i < n; ++i) {
            const int* s = shapes[(rot + i * (1 + rot % 3)) % NS];
            a[i] = OldTn{Mtok, s[0], s[1], s[0] == 4352 ? 4300 : s[0], 0, 0, s[0], s[1], s[1]};
            const KzvTnShape t{Mtok, s[0], s[1], a[i].n_store, s[0], s[1], s[1]};
            own[i] = kzv_tn_group_own_launch(t);
            if (!own[i]) sh[m++] = t;
            const int t256 = kzv_cdiv(t.n_store, 256) * kzv_cdiv(t.K, 256);
            seen_own += own[i]; seen_kept_9_to_23 += !own[i] && t256 >= 9;
        }
        const OldGroup want = old_gemm_tn_group(a, n, sw);
        for (int i = 0; i < n; ++i) CHECK(own[i] == want.own[i]);
        CHECK(m == want.n);
        if (m == 0) continue;
        const KzvTnGroupPlan g = kzv_tn_group_plan(sh, m, sw);
        CHECK(g.n == m && g.grid == want.start[m] && g.start[0] == 0);
        for (int i = 0; i < m; ++i) {
            CHECK(g.splits[i] == want.splits[i] && g.chunk[i] == want.chunk[i] && g.start[i] == want.start[i]);
            CHECK(g.start[i + 1] > g.start[i]);                                                          // Part 3: increasing, ending at the grid
            CHECK(g.start[i + 1] - g.start[i] == kzv_cdiv(sh[i].N, 128) * kzv_cdiv(sh[i].K, 128) * g.splits[i]);
            CHECK((g.splits[i] - 1) * g.chunk[i] < Mtok && (int64_t)g.splits[i] * g.chunk[i] >= Mtok);
        }
        CHECK(g.start[m] == g.grid);
        ++plans;
    }
    CHECK(seen_own > 0 && seen_kept_9_to_23 > 0);      // the 24 is not the 9: both sides of it were planned
    return plans;
}

long sweep_pair() {
    const int Ms[] = {4096, 24576, 33024, 41216}, dims[] = {256, 768, 1536, 2304, 3072};
    long accepted = 0, plans = 0;
    const Var on[] = {{"KZV_PAIR", 1}}, on_r[] = {{"KZV_PAIR", 1}, {"KZV_PAIR_R", 200}}, on_r0[] = {{"KZV_PAIR", 1}, {"KZV_PAIR_R", 0}}, on_min1[] = {{"KZV_PAIR", 1}, {"KZV_NT256P_MIN_TILES", 1000}, {"KZV_TN256_MIN_TILES", 20}};
    const KzvGemmSwitches sws[] = {switches(), switches(on, 1), switches(on_r, 2), switches(on_r0, 2), switches(on_min1, 3)};
    for (const KzvGemmSwitches& sw0 : sws) for (int sched = 0; sched < 2; ++sched) for (int reserve = 0; reserve <= 32; reserve += 32) for (int cus = 256; cus >= 64; cus -= 192)
        for (int M : Ms) for (int Nout : dims) for (int Kin : dims) for (int e : EPIS) {
            KzvGemmSwitches sw = sw0; sw.tn_schedule = sched;
            const KzvGemmEnv env{cus, reserve, 0};
            std::snprintf(g_ctx, sizeof g_ctx, "pair M=%d Nout=%d Kin=%d epi=%d pair=%d pair_r=%d sched=%d reserve=%d cus=%d", M, Nout, Kin, e, sw.pair, sw.pair_r, sched, reserve, cus);
            // dX[M, Kin] = dY[M, Nout] . Wt[Kin, Nout]^T;  dW[Nout, Kin] += dY^T . X[M, Kin]
            const OldNt pn{M, Kin, Nout, Kin, Nout, Nout};
            const OldTn pt{M, Nout, Kin, Nout, 0, 0, Nout, Kin, Kin};
            KzvPairPlan pl;
            const bool got = kzv_pair_plan(KzvNtShape{M, Kin, Nout, Kin, Nout, Nout, e, 2}, KzvTnShape{M, Nout, Kin, Nout, Nout, Kin, Kin}, sw, env, &pl);
            CHECK(got == old_pair_gate(pn, e, pt, sw, env));      // (the levelling never refuses what the gate let through)
            ++plans;
            if (!got) continue;
            ++accepted;
            const int tilesN = (Kin + 255) / 256, tiles = ((M + 255) / 256) * tilesN, tilesKw = (Kin + 255) / 256, tilesNw = (Nout + 255) / 256, per = tilesNw * tilesKw, S = 256 / per;
            const int stages = M / 64;
            CHECK(pl.grid == 256 && pl.tiles == tiles && pl.tilesN == tilesN && pl.per == per && pl.tilesKw == tilesKw && pl.splits == S && pl.strip == sw.nt_strip);
            // Part 3: per weight-gradient tile, the S splits are disjoint ranges of >= 2 stages that cover all stages; every workgroup with a share
            // has the range of its (tile row, split) group; workgroups beyond per * S have none
            int covered[128 * 2]; int owners = 0;
            for (int t = 0; t < per; ++t) {
                int n_splits = 0, sum = 0;
                for (int sp = 0; sp < S; ++sp) covered[sp] = -1;
                for (int b = 0; b < 256; ++b) {
                    if (pl.table.cnt[b] == 0 || pl.table.tile[b] != t) continue;
                    CHECK(pl.table.split[b] < S && covered[pl.table.split[b]] < 0);      // one workgroup per (tile, split)
                    covered[pl.table.split[b]] = b; ++n_splits; ++owners;
                    CHECK(pl.table.cnt[b] >= 2);
                    sum += pl.table.cnt[b];
                }
                CHECK(n_splits == S && sum == stages);
                int next = 0;
                for (int sp = 0; sp < S; ++sp) { const int b = covered[sp]; CHECK(pl.table.t0[b] == next); next += pl.table.cnt[b]; }
                CHECK(next == stages);
            }
            CHECK(owners == per * S);
            for (int b = per * S; b < 256; ++b) CHECK(pl.table.cnt[b] == 0);
            // tiles of one tile ROW and split share the range (the bias gradient is partitioned over them by stage index)
            for (int b = 0; b < per * S; ++b) for (int c = 0; c < per * S; ++c)
                if (pl.table.tile[b] / tilesKw == pl.table.tile[c] / tilesKw && pl.table.split[b] == pl.table.split[c]) CHECK(pl.table.t0[b] == pl.table.t0[c] && pl.table.cnt[b] == pl.table.cnt[c]);
        }
    CHECK(accepted > 0);
    return plans;
}

// ======================================================================================================================================
// Part 2: the benchmark's shapes, 256 CUs, default switches (derived by hand from the chain's text)
// ======================================================================================================================================
KzvNtPlan nt(int M, int N, int K, int epi, int sched = 0, int reserve = 0) {
    KzvGemmSwitches sw = switches();
    sw.nt_schedule = sched;
    std::snprintf(g_ctx, sizeof g_ctx, "named nt (%d,%d,%d) epi=%d sched=%d reserve=%d", M, N, K, epi, sched, reserve);
    return kzv_nt_plan(KzvNtShape{M, N, K, N, K, K, epi, 2}, sw, KzvGemmEnv{256, reserve, 0});
}
KzvTnPlan tn(int N, int K, int reserve = 0) {
    std::snprintf(g_ctx, sizeof g_ctx, "named tn (%d,%d) reserve=%d", N, K, reserve);
    return kzv_tn_plan(KzvTnShape{41216, N, K, N, N, K, K}, switches(), KzvGemmEnv{256, reserve, 0});
}
void named() {
    KzvNtPlan p = nt(24600, 1024, 128, KZV_EPI_F32); CHECK(p.kernel == KZV_GEMM_NT256P && p.grid == 256);
    p = nt(24600, 1024, 128, KZV_EPI_GELU); CHECK(p.kernel == KZV_GEMM_NT256 && p.grid == 388);
    for (int e : EPIS) { p = nt(24600, 1024, 320, e); CHECK(p.kernel == KZV_GEMM_NT256 && p.grid == 388); }
    p = nt(41216, 768, 768, KZV_EPI_BF16); CHECK(p.kernel == KZV_GEMM_NT256P && p.grid == 256);
    p = nt(41216, 768, 768, KZV_EPI_BF16, 1); CHECK(p.kernel == KZV_GEMM_NT256F);
    p = nt(41216, 768, 768, KZV_EPI_BF16, 2); CHECK(p.kernel == KZV_GEMM_NT256H && p.grid == 512);
    p = nt(41216, 768, 768, KZV_EPI_BF16, 0, 32); CHECK(p.kernel == KZV_GEMM_NT256 && p.grid == 483);
    p = nt(41216, 256, 768, KZV_EPI_BF16); CHECK(p.kernel == KZV_GEMM_NT256P && p.grid == 161);
    p = nt(41216, 256, 768, KZV_EPI_BF16, 1); CHECK(p.kernel == KZV_GEMM_NT256P && p.grid == 161);      // 161 < 384: not the free-running kernel
    p = nt(41216, 256, 768, KZV_EPI_GELU); CHECK(p.kernel == KZV_GEMM_NT128 && p.grid == 644);
    KzvTnPlan t = tn(768, 768); CHECK(t.kernel == KZV_GEMM_TN256F && t.tiles == 9 && t.splits == 28 && t.chunk == 23 * 64);
    t = tn(2304, 768); CHECK(t.kernel == KZV_GEMM_TN256F && t.tiles == 27 && t.splits == 9 && t.chunk == 72 * 64);
    t = tn(3072, 768); CHECK(t.kernel == KZV_GEMM_TN256F && t.tiles == 36 && t.splits == 7 && t.chunk == 92 * 64);
    t = tn(768, 3072); CHECK(t.kernel == KZV_GEMM_TN256F && t.tiles == 36 && t.splits == 7 && t.chunk == 92 * 64);
    t = tn(768, 768, 32); CHECK(t.kernel == KZV_GEMM_TN256F && t.tiles == 9 && t.splits == 24 && t.chunk == 27 * 64);
}

// the resolver: defaults, the parse rules that are more than atoi, and "a sentinel written back is read again"
void resolver() {
    std::snprintf(g_ctx, sizeof g_ctx, "resolver");
    KzvGemmSwitches sw = switches();
    CHECK(sw.nt_schedule == 0 && sw.nt_half_mask == 0x3f && sw.nt256p == 1 && sw.nt256p_gelu == 0 && sw.nth_max_k == 1 << 30);
    CHECK(sw.nt256p_min_tiles == 150 && sw.nt256f_min_tiles == 384 && sw.nt256_min_tiles == 384 && sw.nt256h_min_tiles == 768 && sw.nth_stagger == 8);
    CHECK(sw.nt_strip == (3 | 0x100) && sw.rows_max_m == 0 && sw.tn_schedule == 1 && sw.tn256_min_tiles == 9 && sw.pair == 0 && sw.pair_r == -1);
    CHECK(sw.tn_minsteps == 16 && sw.tn_blocks == 512 && sw.nt_grid == 0 && sw.tn_cus == 0);
    const Var v[] = {{"KZV_NT_FREE", 7}, {"KZV_NT_HALF", -1}, {"KZV_NT_STRIP", 256}, {"KZV_BF16_DRAIN", 0}, {"KZV_NT256P_MIN_TILES", 200}, {"KZV_TN_FREE", 5}, {"KZV_PAIR", 9}};
    sw = switches(v, 7);
    CHECK(sw.nt_schedule == 3 && sw.nt_strip == 0 && sw.nt256p_min_tiles == 200 && sw.nt256f_min_tiles == 200 && sw.tn_schedule == 1 && sw.pair == 1);
    sw.nt_schedule = 2; sw.pair = 0;                       // what a setter does ...
    sw.resolve(fake_env);
    CHECK(sw.nt_schedule == 2 && sw.pair == 0);            // ... holds against the environment
    sw.nt_schedule = -1; sw.pair = -1;                     // ... and its -1 has the environment read again
    sw.resolve(fake_env);
    CHECK(sw.nt_schedule == 3 && sw.pair == 1);
}

}  // namespace

int main() {
    resolver();
    const long a = sweep_nt(), b = sweep_tn(), c = sweep_group(), d = sweep_pair();
    named();
    std::printf("gemm_plan: ok (%ld nt, %ld tn, %ld group, %ld pair plans equal to the chain)\n", a, b, c, d);
    return 0;
}
