"""The GEMM dispatch planner (csrc/gemm_plan.h) on the CPU.
(1) tests/host/gemm_plan_main.cpp under AddressSanitizer and UBSan as a stand-alone program, built and run here as a child process (nothing
sanitized is loaded into Python): the planner against the gate-by-gate transcription of the launcher chain it replaced, the benchmark's
shapes by name, and the invariants of token splits, pair tables and group plans.
(2) Through the library: kzv_gemm_nt_plan / kzv_gemm_tn_plan refuse what kzv_gemm_nt / kzv_gemm_tn refuse, with the same code and message,
and the setters move the plan (their -1 puts the default back).  No device is touched: the operands are never read."""
import ctypes as C
import os
import shutil
import subprocess

import pytest

from kzv import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = 0x10000          # a 16-byte aligned address nobody dereferences


def test_planner_equals_the_launcher_chain_under_sanitizers(tmp_path):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.fail("g++ not found: the GEMM planner is tested as a sanitized host program")
    exe = str(tmp_path / "gemm_plan_main")
    # the sanitizer runtimes are linked into the program: it runs the same whatever libraries the environment loads ahead of it
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
           os.path.join(ROOT, "tests", "host", "gemm_plan_main.cpp"), "-o", exe, "-pthread"]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stdout + b.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "gemm_plan: ok" in r.stdout


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(L.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return L.load()


@pytest.fixture
def default_switches(monkeypatch, lib):
    for name in ("KZV_NT_FREE", "KZV_NT_HALF", "KZV_NT_HALF_EPIS", "KZV_NT256P", "KZV_NT256P_MIN_TILES", "KZV_NT256_MIN_TILES", "KZV_NT256H_MIN_TILES",
                 "KZV_NTH_MAX_K", "KZV_NT_GRID", "KZV_ROWS_MAX_M", "KZV_TN_FREE", "KZV_TN256_MIN_TILES", "KZV_TN_CUS", "KZV_CU_RESERVE"):
        monkeypatch.delenv(name, raising=False)
    found = lib.kzv_get_cu_reserve()
    L.check(lib.kzv_set_cu_reserve(0), "set_cu_reserve")
    yield
    L.check(lib.kzv_set_cu_reserve(found), "set_cu_reserve")


def _nt_args(M, N, K, **kw):
    f = dict(A=FAKE, lda=K, B=FAKE, ldb=K, C=FAKE, ldc=N, bias=None, resid=None, ldr=N, aux=None, ldaux=N, M=M, N=N, K=K, n_valid=N, drop_p=0.0, drop_key=0)
    f.update(kw)
    return L.kzv_gemm_nt_args(**f)


def _tn_args(Mtok, N, K, **kw):
    f = dict(P=FAKE, ldp=N, Q=FAKE, ldq=K, OUT=FAKE, ldo=K, Mtok=Mtok, N=N, K=K, n_store=N, dbias=None)
    f.update(kw)
    return L.kzv_gemm_tn_args(**f)


def _nt_plan(lib, a, epi, scope=0, cus=256):
    info = L.kzv_gemm_plan_info()
    L.check(lib.kzv_gemm_nt_plan(C.byref(a), epi, scope, cus, C.byref(info)), "gemm_nt_plan")
    return info


def _tn_plan(lib, a, cus=256):
    info = L.kzv_gemm_plan_info()
    L.check(lib.kzv_gemm_tn_plan(C.byref(a), cus, C.byref(info)), "gemm_tn_plan")
    return info


def test_queries_refuse_what_the_launching_entries_refuse(lib):
    info = L.kzv_gemm_plan_info()
    for a, epi in [(_nt_args(256, 256, 128, A=None), L.EPI_BF16),            # a null operand
                   (_nt_args(256, 256, 96), L.EPI_BF16),                      # K % 64
                   (_nt_args(256, 256, 128), L.EPI_RESID),                    # RESID without resid
                   (_nt_args(256, 256, 128, lda=60), L.EPI_F32),
                   (_nt_args(256, 256, 128), L.EPI_GELU)]:                    # GELU without aux
        rc_q = lib.kzv_gemm_nt_plan(C.byref(a), epi, 0, 256, C.byref(info))
        msg_q = lib.kzv_last_error()
        rc_l = lib.kzv_gemm_nt(C.byref(a), epi, None)                         # refused before anything touches a device
        assert rc_q == rc_l == -1 and msg_q == lib.kzv_last_error() and msg_q.startswith(b"gemm_nt: ")
    for a in [_tn_args(4096, 768, 768, Q=None), _tn_args(4096, 768, 772), _tn_args(0, 768, 768), _tn_args(4096, 768, 768, OUT=FAKE + 4)]:
        rc_q = lib.kzv_gemm_tn_plan(C.byref(a), 256, C.byref(info))
        msg_q = lib.kzv_last_error()
        rc_l = lib.kzv_gemm_tn(C.byref(a), None)
        assert rc_q == rc_l == -1 and msg_q == lib.kzv_last_error() and msg_q.startswith(b"gemm_tn: ")
    assert lib.kzv_gemm_nt_plan(C.byref(_nt_args(256, 256, 128)), 6, 0, 256, C.byref(info)) == -1
    assert lib.kzv_last_error() == b"gemm_nt: unknown epilogue"
    assert lib.kzv_gemm_nt_plan(C.byref(_nt_args(256, 256, 128)), 0, 0, 256, None) == -1


def test_queries_answer_the_benchmark_shapes(lib, default_switches):
    big = _nt_args(41216, 768, 768)
    p = _nt_plan(lib, big, L.EPI_BF16)
    assert (p.kernel, p.grid, p.grid_y, p.block, p.tiles, p.splits, p.chunk) == (L.GEMM_NT256P, 256, 1, 512, 483, 0, 0)
    p = _nt_plan(lib, _nt_args(41216, 3072, 768, aux=FAKE), L.EPI_GELU)
    assert (p.kernel, p.grid, p.block) == (L.GEMM_NT256, 161 * 12, 512)
    p = _nt_plan(lib, _nt_args(41216, 256, 768, aux=FAKE), L.EPI_GELU)
    assert (p.kernel, p.grid, p.block) == (L.GEMM_NT128, 644, 256)
    p = _nt_plan(lib, big, L.EPI_BF16, cus=64)
    assert (p.kernel, p.grid) == (L.GEMM_NT256P, 64)
    small = _nt_args(64, 256, 256)
    assert _nt_plan(lib, small, L.EPI_BF16).kernel == L.GEMM_NT128
    p = _nt_plan(lib, small, L.EPI_BF16, scope=1)                            # inside the generation step
    assert (p.kernel, p.grid, p.grid_y, p.block) == (L.GEMM_ROWS, 4, 4, 256)
    p = _tn_plan(lib, _tn_args(41216, 768, 768))
    assert (p.kernel, p.grid, p.block, p.tiles, p.splits, p.chunk) == (L.GEMM_TN256F, 252, 512, 9, 28, 23 * 64)
    p = _tn_plan(lib, _tn_args(3328, 256, 1024))                              # a decoder weight gradient: 4 tiles of 256x256
    assert (p.kernel, p.block, p.tiles) == (L.GEMM_TN128, 256, 16) and p.grid == 16 * p.splits and p.splits * p.chunk >= 3328


def test_setters_move_the_plan_and_minus_one_puts_the_default_back(lib, default_switches):
    big, small, wgrad = _nt_args(41216, 768, 768), _nt_args(64, 256, 256), _tn_args(41216, 768, 768)
    try:
        L.check(lib.kzv_set_nt_schedule(1), "set_nt_schedule")
        assert _nt_plan(lib, big, L.EPI_BF16).kernel == L.GEMM_NT256F
        L.check(lib.kzv_set_nt_schedule(2), "set_nt_schedule")
        p = _nt_plan(lib, big, L.EPI_BF16)
        assert (p.kernel, p.grid, p.block, p.tiles) == (L.GEMM_NT256H, 512, 256, 966)
        L.check(lib.kzv_set_nt_half_epilogues(1 << L.EPI_F32), "set_nt_half_epilogues")      # ... for the F32 epilogue only
        assert _nt_plan(lib, big, L.EPI_BF16).kernel == L.GEMM_NT256P
        assert _nt_plan(lib, big, L.EPI_F32).kernel == L.GEMM_NT256H
        L.check(lib.kzv_set_nt_half_epilogues(-1), "set_nt_half_epilogues")
        assert _nt_plan(lib, big, L.EPI_BF16).kernel == L.GEMM_NT256H
        L.check(lib.kzv_set_nt_schedule(-1), "set_nt_schedule")
        assert _nt_plan(lib, big, L.EPI_BF16).kernel == L.GEMM_NT256P

        L.check(lib.kzv_set_rows_max_m(1024), "set_rows_max_m")
        assert _nt_plan(lib, small, L.EPI_BF16).kernel == L.GEMM_ROWS
        L.check(lib.kzv_set_rows_max_m(0), "set_rows_max_m")
        assert _nt_plan(lib, small, L.EPI_BF16).kernel == L.GEMM_NT128

        L.check(lib.kzv_set_tn_schedule(0), "set_tn_schedule")
        assert _tn_plan(lib, wgrad).kernel == L.GEMM_TN256
        L.check(lib.kzv_set_tn_schedule(-1), "set_tn_schedule")
        assert _tn_plan(lib, wgrad).kernel == L.GEMM_TN256F

        L.check(lib.kzv_set_cu_reserve(32), "set_cu_reserve")                 # the reserve is an input of the plan
        p = _nt_plan(lib, big, L.EPI_BF16)
        assert (p.kernel, p.grid) == (L.GEMM_NT256, 483)
        p = _tn_plan(lib, wgrad)
        assert (p.splits, p.chunk) == (24, 27 * 64)
    finally:
        lib.kzv_set_nt_schedule(-1)
        lib.kzv_set_nt_half_epilogues(-1)
        lib.kzv_set_rows_max_m(0)
        lib.kzv_set_tn_schedule(-1)
