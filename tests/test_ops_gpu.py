"""Per-op parity of the HIP kernels through the C ABI (include/kzv.h) against fp32 torch math on the same
bf16-rounded inputs.  Tolerances are stated per test; bf16 outputs carry 2^-8 relative rounding."""
import ctypes as C

import numpy as np
import pytest
import torch

from kzv import _lib as L

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module")
def lib():
    return L.load()


def _st():
    return torch.cuda.current_stream().cuda_stream


def _gemm_nt(lib, A, B, epi, bias=None, n_store=None, resid=None, aux=None, drop_p=0.0, key=0):
    M, K = A.shape
    nv = B.shape[0]
    N = n_store or nv
    out = torch.empty(M, N, dtype=torch.float32 if epi in (L.EPI_F32, L.EPI_RESID, 5) else torch.bfloat16, device=DEV)
    a = L.kzv_gemm_nt_args(A=A.data_ptr(), lda=A.stride(0), B=B.data_ptr(), ldb=B.stride(0), C=out.data_ptr(), ldc=N,
                           bias=L.ptr(bias), resid=L.ptr(resid), ldr=N, aux=L.ptr(aux), ldaux=N, M=M, N=N, K=K,
                           n_valid=nv, drop_p=drop_p, drop_key=key)
    L.check(lib.kzv_gemm_nt(C.byref(a), epi, _st()), "gemm_nt")
    return out


def _nt_kernel(lib, M, N, K, nv, epi):
    """the kernel kzv_gemm_nt runs this call on (kzv_gemm_nt_plan: the launching entry's own planner; the operands are never read)"""
    a = L.kzv_gemm_nt_args(A=256, lda=K, B=256, ldb=K, C=256, ldc=N, bias=None, resid=256, ldr=N, aux=256, ldaux=N, M=M, N=N, K=K, n_valid=nv, drop_p=0.0, drop_key=0)
    info = L.kzv_gemm_plan_info()
    L.check(lib.kzv_gemm_nt_plan(C.byref(a), epi, 0, 0, C.byref(info)), "gemm_nt_plan")
    return info


def _tn_kernel(lib, Mt, N, K):
    a = L.kzv_gemm_tn_args(P=256, ldp=N, Q=256, ldq=K, OUT=256, ldo=K, Mtok=Mt, N=N, K=K, n_store=N, dbias=None)
    info = L.kzv_gemm_plan_info()
    L.check(lib.kzv_gemm_tn_plan(C.byref(a), 0, C.byref(info)), "gemm_tn_plan")
    return info


@pytest.fixture(params=["rows", "tiled"])
def small_gemm_kernel(request, lib):
    """threshold 1024: the few-rows kernel of the generation step (gemm_rows.hip); threshold 0 (the default): the same
    shapes through the LDS-staged 128x128 kernel the training step uses for the decoder's GEMMs."""
    L.check(lib.kzv_set_rows_max_m(1024 if request.param == "rows" else 0), "rows_max_m")
    yield request.param
    L.check(lib.kzv_set_rows_max_m(0), "rows_max_m")


@pytest.mark.parametrize("M,N,K", [(128, 128, 64), (200, 132, 128), (483, 384, 192), (1000, 4300, 256), (77, 64, 768), (256, 768, 256), (1, 64, 64)])
def test_gemm_nt_epilogues(lib, small_gemm_kernel, M, N, K):
    torch.manual_seed(M + N + K)
    A = torch.randn(M, K, device=DEV).bfloat16()
    B = (torch.randn(N, K, device=DEV) * 0.1).bfloat16()
    bias = torch.randn(N, device=DEV)
    ref = A.float() @ B.float().t() + bias
    scale = ref.abs().max().item()
    got = _gemm_nt(lib, A, B, L.EPI_F32, bias)
    assert (got - ref).abs().max().item() < 2e-5 * scale + 1e-5          # fp32 accumulate, order differs only
    got = _gemm_nt(lib, A, B, L.EPI_BF16, bias).float()
    assert (got - ref).abs().max().item() < 2 ** -8 * scale               # one bf16 rounding
    aux = torch.empty(M, N, dtype=torch.bfloat16, device=DEV)
    got = _gemm_nt(lib, A, B, L.EPI_GELU, bias, aux=aux).float()
    assert (got - torch.nn.functional.gelu(ref)).abs().max().item() < 2 ** -8 * scale
    xr = ref.double()
    dref = (0.5 * (1 + torch.erf(xr / 2 ** 0.5)) + xr * torch.exp(-0.5 * xr * xr) / (2 * torch.pi) ** 0.5).float()
    assert (aux.float() - dref).abs().max().item() < 2 ** -8 * 1.2                 # aux = gelu'(pre-activation), |gelu'| <= 1.13
    got = _gemm_nt(lib, A, B, 5, bias, aux=aux)
    assert (got - torch.nn.functional.gelu(ref)).abs().max().item() < 2e-5 * scale + 1e-5
    res = torch.randn(M, N, device=DEV)
    got = _gemm_nt(lib, A, B, L.EPI_RESID, bias, resid=res)
    assert (got - ref - res).abs().max().item() < 2e-5 * scale + 1e-5
    # DGELU: C = (A.B^T) * aux, aux = the derivative saved by the forward epilogue
    gp16 = (torch.rand(M, N, device=DEV) * 1.26 - 0.13).bfloat16()
    got = _gemm_nt(lib, A, B, L.EPI_DGELU, None, aux=gp16).float()
    gp = gp16.float().double()
    want = (A.float() @ B.float().t()).double() * gp
    assert (got.double() - want).abs().max().item() < 2 ** -7 * want.abs().max().item()


@pytest.mark.parametrize("M,N,K,nv", [(24600, 1024, 128, 1024), (24600, 1024, 320, 1000), (41216, 768, 768, 768)])
def test_gemm_nt_large_shapes_take_the_256x256_kernel(lib, M, N, K, nv):
    """>= 384 tiles of 256x256 -> the eight-phase kernels (persistent gemm_nt256p.hip for an even K-tile count and
    one-store epilogues, else gemm_nt256.hip): ragged M, odd and minimal K-tile counts, n_valid < N (clamped B rows,
    zeroed columns), all epilogue families."""
    # the docstring's rule, asked of the planner that launches (tests/test_configs_gpu.py runs this test with a CU reserve too: no persistent kernel then)
    persistent = K % 128 == 0 and lib.kzv_get_cu_reserve() == 0
    for epi in (L.EPI_F32, L.EPI_BF16, L.EPI_RESID):
        assert _nt_kernel(lib, M, N, K, nv, epi).kernel == (L.GEMM_NT256P if persistent else L.GEMM_NT256)
    assert _nt_kernel(lib, M, N, K, nv, L.EPI_GELU).kernel == L.GEMM_NT256
    torch.manual_seed(K)
    A = torch.randn(M, K, device=DEV).bfloat16()
    B = (torch.randn(nv, K, device=DEV) * 0.1).bfloat16()
    bias = torch.randn(nv, device=DEV)
    ref = A.float() @ B.float().t() + bias
    scale = ref.abs().max().item()
    got = _gemm_nt(lib, A, B, L.EPI_F32, bias, n_store=N)
    assert (got[:, :nv] - ref).abs().max().item() < 2e-5 * scale + 1e-5
    assert torch.all(got[:, nv:] == 0)
    got = _gemm_nt(lib, A, B, L.EPI_BF16, bias, n_store=N).float()
    assert (got[:, :nv] - ref).abs().max().item() < 2 ** -8 * scale
    res = torch.randn(M, N, device=DEV)
    got = _gemm_nt(lib, A, B, L.EPI_RESID, bias, n_store=N, resid=res)
    assert (got[:, :nv] - ref - res[:, :nv]).abs().max().item() < 2e-5 * scale + 1e-5
    aux = torch.empty(M, N, dtype=torch.bfloat16, device=DEV)
    got = _gemm_nt(lib, A, B, L.EPI_GELU, bias, n_store=N, aux=aux).float()
    assert (got[:, :nv] - torch.nn.functional.gelu(ref)).abs().max().item() < 2 ** -8 * scale
    xr = ref.double()
    dref = (0.5 * (1 + torch.erf(xr / 2 ** 0.5)) + xr * torch.exp(-0.5 * xr * xr) / (2 * torch.pi) ** 0.5).float()
    assert (aux[:, :nv].float() - dref).abs().max().item() < 2 ** -8 * 1.2          # aux = gelu'(pre-activation)
    # run-to-run determinism (a staging race would show up as rare differing tiles)
    first = _gemm_nt(lib, A, B, L.EPI_F32, bias, n_store=N)
    for _ in range(5):
        assert torch.equal(_gemm_nt(lib, A, B, L.EPI_F32, bias, n_store=N), first)


@pytest.mark.parametrize("M,N,K,nv,epi", [(41216, 768, 768, 768, "bf16"), (24600, 1024, 256, 1000, "resid"), (24600, 1024, 128, 1024, "f32"), (33024, 768, 1536, 768, "dgelu")])
def test_gemm_nt_free_running_schedule_is_bit_identical_to_the_ping_pong(lib, M, N, K, nv, epi):
    """kzv_set_nt_schedule(1): the persistent 256x256 kernel on the free-running K loop (gemm_nt256f.hip: two barriers per K-tile,
    every wave's loads under its own MFMAs -- round 4's prototype of VERDICT r03 item 1; slower than the eight-phase ping-pong on
    this operand geometry, so it is not the default, but it is the schedule the weight-gradient kernel now runs).  Same per-
    accumulator summation order, so the same bits: interior and edge tiles, n_valid < N, every one-store epilogue family, a
    two-K-tile reduction, and six repeats (a staging race would show as rare differing tiles)."""
    torch.manual_seed(M + K)
    A = torch.randn(M, K, device=DEV).bfloat16()
    B = (torch.randn(nv, K, device=DEV) * 0.1).bfloat16()
    bias = torch.randn(nv, device=DEV)
    res = torch.randn(M, N, device=DEV) if epi == "resid" else None
    aux = (torch.rand(M, N, device=DEV) * 1.2).bfloat16() if epi == "dgelu" else None
    code = {"bf16": L.EPI_BF16, "f32": L.EPI_F32, "resid": L.EPI_RESID, "dgelu": L.EPI_DGELU}[epi]
    kw = dict(bias=None if epi == "dgelu" else bias, n_store=N, resid=res, aux=aux, drop_p=0.1 if epi == "resid" else 0.0, key=11)
    try:
        L.check(lib.kzv_set_nt_schedule(0), "set_nt_schedule")
        assert _nt_kernel(lib, M, N, K, nv, code).kernel == L.GEMM_NT256P
        ref = _gemm_nt(lib, A, B, code, **kw)
        L.check(lib.kzv_set_nt_schedule(1), "set_nt_schedule")
        assert _nt_kernel(lib, M, N, K, nv, code).kernel == L.GEMM_NT256F
        for _ in range(6):
            assert torch.equal(_gemm_nt(lib, A, B, code, **kw), ref)
    finally:
        L.check(lib.kzv_set_nt_schedule(-1), "set_nt_schedule")


@pytest.mark.parametrize("M,N,K,nv,epi", [(41216, 768, 768, 768, "bf16"), (24600, 1024, 384, 1000, "resid"), (24600, 1024, 384, 1000, "gelu"),
                                          (24600, 1024, 768, 1024, "f32"), (33024, 768, 1536, 768, "dgelu")])
def test_gemm_nt_four_wave_kernel_is_bit_identical_to_the_256x256_kernels(lib, M, N, K, nv, epi):
    """kzv_set_nt_schedule(2): the 256x128 kernel of four waves, two workgroups per CU (gemm_nt256h.hip; round 4's build of VERDICT
    r03 item 3: one workgroup's drain under the other's K loop).  Not the default -- its three-group LDS ring leaves the K loop
    latency-bound, profiles/r04_kloop_ablation.md section 4 -- but it is the same arithmetic in the same order: interior and edge
    tiles, n_valid < N, both outputs of the GELU epilogue, six repeats."""
    torch.manual_seed(M + K)
    A = torch.randn(M, K, device=DEV).bfloat16()
    B = (torch.randn(nv, K, device=DEV) * 0.1).bfloat16()
    bias = torch.randn(nv, device=DEV)
    res = torch.randn(M, N, device=DEV) if epi == "resid" else None
    aux = (torch.rand(M, N, device=DEV) * 1.2).bfloat16() if epi == "dgelu" else torch.zeros(M, N, dtype=torch.bfloat16, device=DEV) if epi == "gelu" else None
    code = {"bf16": L.EPI_BF16, "f32": L.EPI_F32, "resid": L.EPI_RESID, "dgelu": L.EPI_DGELU, "gelu": L.EPI_GELU}[epi]
    kw = dict(bias=None if epi == "dgelu" else bias, n_store=N, resid=res, aux=aux, drop_p=0.1 if epi == "resid" else 0.0, key=11)
    try:
        L.check(lib.kzv_set_nt_schedule(0), "set_nt_schedule")
        assert _nt_kernel(lib, M, N, K, nv, code).kernel == (L.GEMM_NT256 if epi == "gelu" else L.GEMM_NT256P)
        ref = _gemm_nt(lib, A, B, code, **kw)
        ref_aux = aux.clone() if epi == "gelu" else None
        L.check(lib.kzv_set_nt_schedule(2), "set_nt_schedule")
        assert _nt_kernel(lib, M, N, K, nv, code).kernel == L.GEMM_NT256H
        for _ in range(6):
            if epi == "gelu":
                aux.zero_()
            assert torch.equal(_gemm_nt(lib, A, B, code, **kw), ref)
            if epi == "gelu":
                assert torch.equal(aux, ref_aux)
    finally:
        L.check(lib.kzv_set_nt_schedule(-1), "set_nt_schedule")


def test_gemm_nt_padded_columns_are_zero(lib, small_gemm_kernel):
    A = torch.randn(130, 64, device=DEV).bfloat16()
    B = torch.randn(157, 64, device=DEV).bfloat16()
    bias = torch.randn(157, device=DEV)
    got = _gemm_nt(lib, A, B, L.EPI_F32, bias, n_store=192)
    assert torch.all(got[:, 157:] == 0)
    assert (got[:, :157] - (A.float() @ B.float().t() + bias)).abs().max().item() < 1e-3


def test_gemm_nt_dropout_statistics_and_determinism(lib):
    M, N, K = 512, 768, 64
    A = torch.zeros(M, K, device=DEV).bfloat16()
    B = torch.zeros(N, K, device=DEV).bfloat16()
    bias = torch.ones(N, device=DEV)
    res = torch.zeros(M, N, device=DEV)
    a = _gemm_nt(lib, A, B, L.EPI_RESID, bias, resid=res, drop_p=0.1, key=1234)
    b = _gemm_nt(lib, A, B, L.EPI_RESID, bias, resid=res, drop_p=0.1, key=1234)
    c = _gemm_nt(lib, A, B, L.EPI_RESID, bias, resid=res, drop_p=0.1, key=99)
    assert torch.equal(a, b) and not torch.equal(a, c)
    kept = a != 0
    frac = 1 - kept.float().mean().item()
    assert abs(frac - 0.1) < 0.005                                        # 393k samples: sigma ~ 0.0005
    assert abs(a[kept].mean().item() - 1 / 0.9) < 1e-3                    # inverted-dropout scale
    # no row/column structure
    assert (1 - kept.float().mean(0)).sub(0.1).abs().max().item() < 0.06


@pytest.mark.parametrize("Mt,N,K", [(64, 128, 128), (200, 136, 64), (1000, 256, 384), (3000, 4352, 256), (41, 64, 64)])
def test_gemm_tn(lib, Mt, N, K):
    torch.manual_seed(Mt)
    Pm = torch.randn(Mt, N, device=DEV).bfloat16()
    Q = torch.randn(Mt, K, device=DEV).bfloat16()
    base = torch.randn(N, K, device=DEV)
    out = base.clone()
    db0 = torch.randn(N, device=DEV)
    db = db0.clone()
    a = L.kzv_gemm_tn_args(P=Pm.data_ptr(), ldp=N, Q=Q.data_ptr(), ldq=K, OUT=out.data_ptr(), ldo=K, Mtok=Mt, N=N, K=K, n_store=N,
                           dbias=db.data_ptr())
    L.check(lib.kzv_gemm_tn(C.byref(a), _st()), "gemm_tn")
    ref = Pm.float().t() @ Q.float() + base
    assert (out - ref).abs().max().item() < 1e-5 * ref.abs().max().item() + 1e-4     # accumulates INTO out
    # fused bias gradient: dbias += column sums of P (each token counted exactly once across k-tiles and splits)
    assert (db - db0 - Pm.float().sum(0)).abs().max().item() < 1e-3


@pytest.mark.parametrize("Mt,N,K", [(8192, 1536, 1024), (4096, 2304, 768), (4160, 1288, 1280)])
def test_gemm_tn_large_outputs_take_the_256x256_kernel(lib, Mt, N, K):
    """>= 9 output tiles of 256x256 and Mtok % 64 == 0 -> gemm_tn256.hip (eight-phase schedule, token splits, atomics
    epilogue, VALU bias sums); ragged N / K (clamped columns, guarded stores) in the last case; accumulates INTO out."""
    assert _tn_kernel(lib, Mt, N, K).kernel == L.GEMM_TN256F
    torch.manual_seed(Mt + N)
    Pm = torch.randn(Mt, N, device=DEV).bfloat16()
    Q = torch.randn(Mt, K, device=DEV).bfloat16()
    base = torch.randn(N, K, device=DEV)
    out = base.clone()
    db0 = torch.randn(N, device=DEV)
    db = db0.clone()
    a = L.kzv_gemm_tn_args(P=Pm.data_ptr(), ldp=N, Q=Q.data_ptr(), ldq=K, OUT=out.data_ptr(), ldo=K, Mtok=Mt, N=N, K=K, n_store=N,
                           dbias=db.data_ptr())
    L.check(lib.kzv_gemm_tn(C.byref(a), _st()), "gemm_tn")
    ref = Pm.float().t() @ Q.float() + base
    # fp32 sums of 512-token splits; each split's partial tile crosses the workspace rounded to bf16 (2^-9 of ITS magnitude, a
    # 1 / sqrt(splits) share of the sum; observed 0.7 - 1.7e-3 of the largest entry) -- the reference's autocast GEMM rounds the whole
    # weight gradient to bf16 (4e-3)
    assert (out - ref).abs().max().item() < 4e-3 * ref.abs().max().item() + 2e-3
    assert (db - db0 - Pm.float().sum(0)).abs().max().item() < 2e-3 * (Mt / 4096) ** 0.5 + 2e-3
    # the partial tiles are folded in a fixed order: bit-identical from run to run (a staging race would show up as
    # rare differing tiles)
    for _ in range(5):
        again = base.clone()
        a.OUT = again.data_ptr()
        L.check(lib.kzv_gemm_tn(C.byref(a), _st()), "gemm_tn")
        assert torch.equal(again, out)


@pytest.mark.parametrize("Nout,Kin,epi", [(768, 3072, "dgelu"), (2304, 768, "bf16"), (768, 768, "f32")])
def test_dgrad_wgrad_pair_launch_equals_the_two_launches(lib, Nout, Kin, epi):
    """kzv_gemm_dgrad_wgrad with the pair kernel on (kzv_set_pair(1); off by default): the input gradient is bit-identical
    to kzv_gemm_nt's, the weight gradient within the bf16-partial tolerance of fp32 math (its token splits differ from kzv_gemm_tn's),
    the bias gradient equal to 1e-5; accumulates INTO dW; run-to-run identical."""
    M = 33024
    torch.manual_seed(Nout + Kin)
    dY = torch.randn(M, Nout, device=DEV).bfloat16(); X = torch.randn(M, Kin, device=DEV).bfloat16()
    Wt = (torch.randn(Kin, Nout, device=DEV) * 0.05).bfloat16()
    dt = torch.float32 if epi == "f32" else torch.bfloat16
    dX = torch.empty(M, Kin, dtype=dt, device=DEV)
    aux = (torch.rand(M, Kin, device=DEV) * 1.2).bfloat16() if epi == "dgelu" else None
    base = torch.randn(Nout, Kin, device=DEV)
    code = {"bf16": L.EPI_BF16, "f32": L.EPI_F32, "dgelu": L.EPI_DGELU}[epi]

    def run(pair):
        dW, db = base.clone(), torch.zeros(Nout, device=DEV)
        na = L.kzv_gemm_nt_args(A=dY.data_ptr(), lda=Nout, B=Wt.data_ptr(), ldb=Nout, C=dX.data_ptr(), ldc=Kin, bias=None, resid=None, ldr=Kin,
                                aux=L.ptr(aux), ldaux=Kin, M=M, N=Kin, K=Nout, n_valid=Kin, drop_p=0.0, drop_key=0)
        ta = L.kzv_gemm_tn_args(P=dY.data_ptr(), ldp=Nout, Q=X.data_ptr(), ldq=Kin, OUT=dW.data_ptr(), ldo=Kin, Mtok=M, N=Nout, K=Kin, n_store=Nout, dbias=db.data_ptr())
        L.check(lib.kzv_set_pair(pair), "set_pair")
        half_nt, half_tn = _nt_kernel(lib, M, Kin, Nout, Kin, code), _tn_kernel(lib, M, Nout, Kin)
        assert (half_nt.kernel, half_tn.kernel) == (L.GEMM_NT256P, L.GEMM_TN256F)      # what the two launches run on ...
        assert (half_nt.pair, half_tn.pair) == (pair, pair)                             # ... and both halves accept the one-launch form when it is on
        dX.zero_()
        L.check(lib.kzv_gemm_dgrad_wgrad(C.byref(na), code, C.byref(ta), _st()), "dgrad_wgrad")
        torch.cuda.synchronize()
        return dX.clone(), dW, db
    try:
        sx, sw, sb = run(0)
        px, pw, pb = run(1)
        px2, pw2, _ = run(1)
    finally:
        L.check(lib.kzv_set_pair(-1), "set_pair")
    assert torch.equal(px, sx) and torch.equal(px2, px) and torch.equal(pw2, pw)
    want = dY.float().t() @ X.float() + base
    assert (pw - want).abs().max().item() < 4e-3 * want.abs().max().item() + 2e-3
    assert (pb - sb).abs().max().item() < 1e-5 * sb.abs().max().item() + 1e-4


@pytest.mark.parametrize("schedule", [0, 1])
def test_gemm_tn256_schedules_agree_bit_for_bit_and_cancelling_partials_are_bounded(lib, schedule):
    """(1) The free-running stage schedule (kzv_set_tn_schedule(1), the default since round 4) and the eight-phase ping-pong produce
    the SAME bits: every accumulator sums its stages in the same order.
    (2) ADVICE r03: the token splits' partial tiles cross the workspace as bf16, each rounded once (2^-9 of ITS magnitude).  When
    the partials CANCEL, that is an error relative to the partials, not to the (small) final gradient: here the second half of the
    tokens carries the negated rows of the first half (x 0.999), so every partial is ~1000 x the final sum.  Stated bound: the
    absolute error stays below 2^-8 x sqrt(splits) x the largest |partial| entry -- about 0.5 of the final gradient's largest
    entry in this construction (an fp32-partial build, -DKZV_TN_F32_PARTIALS, gives ~1e-4 here), and within 4e-3 of it whenever
    the partials do not cancel (the test above).  Gradients of a training step are sums of same-signed-on-average token
    contributions scaled by 1 / count; the loss-curve equivalence of the two builds is recorded in DESIGN.md section 4."""
    Mt, N, K = 8192, 1536, 1024
    torch.manual_seed(7)
    half_p = torch.randn(Mt // 2, N, device=DEV)
    Pm = torch.cat([half_p, -0.999 * half_p]).bfloat16()
    half_q = torch.randn(Mt // 2, K, device=DEV).bfloat16()
    Q = torch.cat([half_q, half_q])
    out = torch.zeros(N, K, device=DEV)
    a = L.kzv_gemm_tn_args(P=Pm.data_ptr(), ldp=N, Q=Q.data_ptr(), ldq=K, OUT=out.data_ptr(), ldo=K, Mtok=Mt, N=N, K=K, n_store=N, dbias=None)
    try:
        L.check(lib.kzv_set_tn_schedule(schedule), "set_tn_schedule")
        L.check(lib.kzv_gemm_tn(C.byref(a), _st()), "gemm_tn")
        other = torch.zeros(N, K, device=DEV)
        a.OUT = other.data_ptr()
        L.check(lib.kzv_set_tn_schedule(1 - schedule), "set_tn_schedule")
        L.check(lib.kzv_gemm_tn(C.byref(a), _st()), "gemm_tn")
    finally:
        L.check(lib.kzv_set_tn_schedule(-1), "set_tn_schedule")
    assert torch.equal(out, other)
    ref = Pm.double().t() @ Q.double()
    partial = (Pm[:Mt // 2].double().t() @ Q[:Mt // 2].double()).abs().max().item()          # magnitude of what cancels
    splits = 256 // ((N // 256) * (K // 256))
    err = (out.double() - ref).abs().max().item()
    assert err < 2 ** -8 * splits ** 0.5 * partial, (err, partial, ref.abs().max().item())
    assert ref.abs().max().item() < 5e-3 * partial                                             # the construction does cancel


@pytest.mark.parametrize("rows,H", [(7, 64), (1000, 256), (333, 768), (64, 1024)])
def test_layernorm_fwd_bwd(lib, rows, H):
    torch.manual_seed(rows)
    x = (torch.randn(rows, H, device=DEV) * 2 + 0.5).requires_grad_(True)
    g = (1 + 0.1 * torch.randn(H, device=DEV)).requires_grad_(True)
    b = (0.1 * torch.randn(H, device=DEV)).requires_grad_(True)
    y16 = torch.empty(rows, H, dtype=torch.bfloat16, device=DEV)
    y32 = torch.empty(rows, H, device=DEV)
    stats = torch.empty(rows, 2, device=DEV)
    L.check(lib.kzv_layernorm_fwd(x.data_ptr(), g.data_ptr(), b.data_ptr(), y16.data_ptr(), y32.data_ptr(), stats.data_ptr(),
                                  rows, H, 1e-12, _st()), "ln_fwd")
    ref = torch.nn.functional.layer_norm(x, (H,), g, b, 1e-12)
    assert (y32 - ref).abs().max().item() < 2e-5
    assert (y16.float() - ref).abs().max().item() < 2 ** -8 * ref.abs().max().item()
    dy = torch.randn(rows, H, device=DEV)
    ref.backward(dy)
    for dy_in, is32, tol in ((dy, 1, 3e-5), (dy.bfloat16(), 0, 0.02)):
        dx = torch.ones(rows, H, device=DEV)
        dg = torch.zeros(H, device=DEV)
        db = torch.zeros(H, device=DEV)
        L.check(lib.kzv_layernorm_bwd(dy_in.data_ptr(), is32, x.data_ptr(), stats.data_ptr(), g.data_ptr(), dx.data_ptr(), 1,
                                      dg.data_ptr(), db.data_ptr(), rows, H, _st()), "ln_bwd")
        assert (dx - 1 - x.grad).abs().max().item() < tol * max(1.0, x.grad.abs().max().item())      # accumulate_dx
        assert (dg - g.grad).abs().max().item() < tol * max(1.0, g.grad.abs().max().item()) * 4
        assert (db - b.grad).abs().max().item() < tol * max(1.0, b.grad.abs().max().item()) * 4


def _attn_ref(q, k, v, heads, mask):
    B, Sq, H = q.shape
    Sk = k.shape[1]
    qh = q.view(B, Sq, heads, 64).transpose(1, 2)
    kh = k.view(B, Sk, heads, 64).transpose(1, 2)
    vh = v.view(B, Sk, heads, 64).transpose(1, 2)
    s = qh @ kh.transpose(2, 3) * 0.125
    if mask is not None:
        s = s.masked_fill(~mask, float("-inf"))
    p = torch.softmax(s, -1)
    return (p @ vh).transpose(1, 2).reshape(B, Sq, H)


@pytest.mark.parametrize("B,heads,Sq,Sk,mode", [(2, 2, 9, 9, 0), (3, 12, 161, 161, 0), (2, 4, 127, 160, 0),
                                                (3, 4, 127, 127, 1), (2, 1, 23, 23, 1), (1, 3, 192, 192, 0),
                                                # > 192 tokens: the reference's default 1024x64 columns (257 tokens),
                                                # cross attention over 256 patches, and the 288-token maximum
                                                (2, 3, 257, 257, 0), (2, 4, 127, 256, 0), (1, 2, 288, 288, 0), (1, 1, 193, 40, 0)])
def test_attention_fwd_bwd(lib, B, heads, Sq, Sk, mode):
    torch.manual_seed(Sq * 7 + Sk)
    H = heads * 64
    # packed layouts like the model's: q | k | v columns of one buffer when self-attention
    q = torch.randn(B, Sq, H, device=DEV).bfloat16()
    k = torch.randn(B, Sk, H, device=DEV).bfloat16()
    v = torch.randn(B, Sk, H, device=DEV).bfloat16()
    ids = None
    mask = None
    if mode == 1:
        ids = torch.randint(5, 50, (B, Sk + 1), device=DEV, dtype=torch.int64)
        for b in range(B):
            ids[b, 3 + 5 * b:] = 1                       # pad tail (pad id 1); first tokens valid
        causal = torch.ones(Sq, Sk, dtype=torch.bool, device=DEV).tril()
        mask = causal[None, None] & (ids[:, :Sk] != 1)[:, None, None, :]
    qf, kf, vf = (t.float().requires_grad_(True) for t in (q, k, v))
    ref = _attn_ref(qf, kf, vf, heads, mask)
    do = torch.randn(B, Sq, H, device=DEV).bfloat16()
    ref.backward(do.float())
    o = torch.empty(B, Sq, H, dtype=torch.bfloat16, device=DEV)
    lse = torch.empty(B, heads, Sq, device=DEV)
    dq, dk, dv = torch.zeros_like(q), torch.zeros_like(k), torch.zeros_like(v)
    a = L.kzv_attn_args(Q=q.data_ptr(), K=k.data_ptr(), V=v.data_ptr(), O=o.data_ptr(), LSE=lse.data_ptr(),
                        dO=do.data_ptr(), dQ=dq.data_ptr(), dK=dk.data_ptr(), dV=dv.data_ptr(),
                        ldq=H, ldk=H, ldv=H, ldo=H, ids=L.ptr(ids), ld_ids=Sk + 1, pad_id=1,
                        B=B, heads=heads, Sq=Sq, Sk=Sk, mode=mode, drop_p=0.0, drop_key=0)
    L.check(lib.kzv_attn_fwd(C.byref(a), _st()), "attn_fwd")
    L.check(lib.kzv_attn_bwd(C.byref(a), _st()), "attn_bwd")
    # tolerance: P and the outputs are rounded to bf16 (2^-8 rel) before/after 64..192-term sums
    assert (o.float() - ref).abs().max().item() < 0.02 * max(1.0, ref.abs().max().item())
    for got, want, name in ((dq, qf.grad, "dq"), (dk, kf.grad, "dk"), (dv, vf.grad, "dv")):
        err = (got.float() - want).abs().max().item()
        assert err < 0.03 * max(1.0, want.abs().max().item()), (name, err)
    # LSE = logsumexp of the scaled, masked scores
    qh = q.float().view(B, Sq, heads, 64).transpose(1, 2)
    kh = k.float().view(B, Sk, heads, 64).transpose(1, 2)
    s = qh @ kh.transpose(2, 3) * 0.125
    if mask is not None:
        s = s.masked_fill(~mask, float("-inf"))
    assert (lse - torch.logsumexp(s, -1)).abs().max().item() < 2e-3


@pytest.mark.parametrize("pairs,Sq,Sk,p", [(5, 161, 161, 0.1), (3, 60, 160, 0.1), (2, 7, 5, 0.5), (1, 257, 257, 0.25), (4, 33, 18, 0.0)])
def test_attention_dropout_mask_entry_equals_the_numpy_statement(lib, pairs, Sq, Sk, p):
    """kzv_debug_attn_dropout_mask (the device generator, scalar form) bit for bit against oracle/attn_dropout.py."""
    from oracle import attn_dropout as AD
    out = torch.empty(pairs * Sq, Sk, device=DEV)
    for key in (0, 0xdeadbeef, 12345):
        L.check(lib.kzv_debug_attn_dropout_mask(key, p, pairs, Sq, Sk, out.data_ptr(), _st()), "mask")
        assert np.array_equal(out.cpu().numpy(), AD.multiplier(key, p, pairs, Sq, Sk)), key


@pytest.mark.parametrize("B,heads,Sq,Sk,mode,drop", [(3, 12, 161, 161, 0, 0.1), (2, 4, 60, 160, 0, 0.1), (2, 4, 127, 160, 0, 0.3),
                                                     (3, 4, 60, 60, 1, 0.1), (2, 2, 127, 127, 1, 0.1), (2, 3, 100, 100, 0, 0.1),
                                                     (2, 3, 257, 257, 0, 0.1), (1, 2, 192, 176, 0, 0.1), (2, 2, 16, 16, 0, 0.1)])
def test_attention_fwd_bwd_with_dropout_against_explicit_masks(lib, B, heads, Sq, Sk, mode, drop):
    """Dropout ON, every instance of the MFMA kernels (exact 11- and 10-tile, generic <= 192 and <= 288, causal): the PACKED
    generator inside the kernels (forward: 4 keys of one query per lane; backward: 4 queries of one key) must draw exactly the
    masks the scalar debug entry reports -- forward output and all three gradients against fp32 torch math on those masks."""
    torch.manual_seed(Sq * 3 + Sk + mode)
    H = heads * 64
    q = torch.randn(B, Sq, H, device=DEV).bfloat16()
    k = torch.randn(B, Sk, H, device=DEV).bfloat16()
    v = torch.randn(B, Sk, H, device=DEV).bfloat16()
    ids, amask = None, None
    if mode == 1:
        ids = torch.randint(5, 50, (B, Sk + 1), device=DEV, dtype=torch.int64)
        for b in range(B):
            ids[b, Sk - 2 - 5 * b:] = 1
        amask = torch.ones(Sq, Sk, dtype=torch.bool, device=DEV).tril()[None, None] & (ids[:, :Sk] != 1)[:, None, None, :]
    key = 77 + Sq
    dmask = torch.empty(B * heads * Sq, Sk, device=DEV)
    L.check(lib.kzv_debug_attn_dropout_mask(key, drop, B * heads, Sq, Sk, dmask.data_ptr(), _st()), "mask")
    dmask = dmask.view(B, heads, Sq, Sk)
    assert 0.5 * drop < (dmask == 0).float().mean().item() < 1.5 * drop
    qf, kf, vf = (t.float().requires_grad_(True) for t in (q, k, v))
    qh, kh, vh = (t.view(B, -1, heads, 64).transpose(1, 2) for t in (qf, kf, vf))
    sc = qh @ kh.transpose(2, 3) * 0.125
    if amask is not None:
        sc = sc.masked_fill(~amask, float("-inf"))
    ref = ((torch.softmax(sc, -1) * dmask) @ vh).transpose(1, 2).reshape(B, Sq, H)
    do = torch.randn(B, Sq, H, device=DEV).bfloat16()
    ref.backward(do.float())
    o = torch.empty(B, Sq, H, dtype=torch.bfloat16, device=DEV)
    lse = torch.empty(B, heads, Sq, device=DEV)
    dq, dk, dv = torch.zeros_like(q), torch.zeros_like(k), torch.zeros_like(v)
    a = L.kzv_attn_args(Q=q.data_ptr(), K=k.data_ptr(), V=v.data_ptr(), O=o.data_ptr(), LSE=lse.data_ptr(),
                        dO=do.data_ptr(), dQ=dq.data_ptr(), dK=dk.data_ptr(), dV=dv.data_ptr(),
                        ldq=H, ldk=H, ldv=H, ldo=H, ids=L.ptr(ids), ld_ids=Sk + 1, pad_id=1,
                        B=B, heads=heads, Sq=Sq, Sk=Sk, mode=mode, drop_p=drop, drop_key=key)
    L.check(lib.kzv_attn_fwd(C.byref(a), _st()), "attn_fwd")
    L.check(lib.kzv_attn_bwd(C.byref(a), _st()), "attn_bwd")
    # one wrong mask bit moves an output by ~ |v| / Sk >> the bf16 tolerance below
    assert (o.float() - ref).abs().max().item() < 0.02 * max(1.0, ref.abs().max().item())
    for got, want, name in ((dq, qf.grad, "dq"), (dk, kf.grad, "dk"), (dv, vf.grad, "dv")):
        err = (got.float() - want).abs().max().item()
        assert err < 0.03 * max(1.0, want.abs().max().item()), (name, err)
    assert (lse - torch.logsumexp(sc, -1)).abs().max().item() < 2e-3         # the log-sum-exp is of the UN-dropped scores


def test_attention_dropout_consistent_between_fwd_and_bwd(lib):
    """With dropout on, backward must regenerate the forward's mask: check dV = P_d^T dO through a
    finite-difference-free identity -- run fwd twice with V=e_j probes is overkill; instead verify
    determinism and that E[O] over keys matches the no-dropout output within sampling error."""
    torch.manual_seed(5)
    B, heads, S = 8, 4, 161
    H = heads * 64
    q = (torch.randn(B, S, H, device=DEV) * 0.3).bfloat16()
    k = (torch.randn(B, S, H, device=DEV) * 0.3).bfloat16()
    v = torch.randn(B, S, H, device=DEV).bfloat16()
    outs = []
    for p, key in ((0.0, 0), (0.1, 11), (0.1, 11), (0.1, 12)):
        o = torch.empty(B, S, H, dtype=torch.bfloat16, device=DEV)
        lse = torch.empty(B, heads, S, device=DEV)
        a = L.kzv_attn_args(Q=q.data_ptr(), K=k.data_ptr(), V=v.data_ptr(), O=o.data_ptr(), LSE=lse.data_ptr(),
                            ldq=H, ldk=H, ldv=H, ldo=H, B=B, heads=heads, Sq=S, Sk=S, mode=0, drop_p=p, drop_key=key)
        L.check(lib.kzv_attn_fwd(C.byref(a), _st()), "attn_fwd")
        outs.append(o.float())
    assert torch.equal(outs[1], outs[2]) and not torch.equal(outs[1], outs[3])
    # O is linear in V for a fixed mask, so <dO, O> == <dV, V> iff backward regenerates the forward's mask
    do = torch.randn(B, S, H, device=DEV).bfloat16()
    dq, dk, dv = torch.zeros_like(q), torch.zeros_like(k), torch.zeros_like(v)
    o = torch.empty(B, S, H, dtype=torch.bfloat16, device=DEV)
    a = L.kzv_attn_args(Q=q.data_ptr(), K=k.data_ptr(), V=v.data_ptr(), O=o.data_ptr(), LSE=lse.data_ptr(),
                        dO=do.data_ptr(), dQ=dq.data_ptr(), dK=dk.data_ptr(), dV=dv.data_ptr(),
                        ldq=H, ldk=H, ldv=H, ldo=H, B=B, heads=heads, Sq=S, Sk=S, mode=0, drop_p=0.1, drop_key=11)
    L.check(lib.kzv_attn_fwd(C.byref(a), _st()), "attn_fwd")
    L.check(lib.kzv_attn_bwd(C.byref(a), _st()), "attn_bwd")
    lhs = (do.double() * o.double()).sum().item()
    rhs = (dv.double() * v.double()).sum().item()
    scale = (do.double().abs() * o.double().abs()).sum().item()
    assert abs(lhs - rhs) < 2e-3 * scale, (lhs, rhs, scale)
    # dropout is unbiased: mean difference over 330k outputs ~ 0
    assert (outs[1] - outs[0]).mean().abs().item() < 2e-3
    rel = (outs[1] - outs[0]).std().item() / outs[0].std().item()
    assert 0.1 < rel < 1.0


@pytest.mark.parametrize("B,heads,S,D,drop", [(2, 3, 37, 96, 0.0), (2, 2, 257, 96, 0.1), (1, 4, 70, 32, 0.1), (1, 1, 161, 128, 0.0)])
def test_attention_other_head_dims_fwd_bwd(lib, B, heads, S, D, drop):
    """head_dim != 64 (the reference CLI's default ViT: 768 / 8 heads = 96) runs on the plain fp32 kernel of
    attention_generic.hip: forward and backward against fp32 torch math, with the dropout mask the library reports."""
    torch.manual_seed(S + D)
    H = heads * D
    qkv = (torch.randn(B * S, 3 * H, device=DEV) * 0.5).bfloat16()
    dO = (torch.randn(B * S, H, device=DEV) * 0.5).bfloat16()
    O = torch.empty(B * S, H, dtype=torch.bfloat16, device=DEV)
    lse = torch.empty(B, heads, S, device=DEV)
    dqkv = torch.zeros_like(qkv)
    key = 1234
    a = L.kzv_attn_args(Q=qkv.data_ptr(), K=qkv[:, H:].data_ptr(), V=qkv[:, 2 * H:].data_ptr(), O=O.data_ptr(), LSE=lse.data_ptr(),
                        dO=dO.data_ptr(), dQ=dqkv.data_ptr(), dK=dqkv[:, H:].data_ptr(), dV=dqkv[:, 2 * H:].data_ptr(),
                        ldq=3 * H, ldk=3 * H, ldv=3 * H, ldo=H, ids=None, ld_ids=0, pad_id=1, B=B, heads=heads, Sq=S, Sk=S, mode=0,
                        drop_p=drop, drop_key=key, head_dim=D)
    L.check(lib.kzv_attn_fwd(C.byref(a), _st()), "attn_fwd")
    L.check(lib.kzv_attn_bwd(C.byref(a), _st()), "attn_bwd")
    mask = torch.ones(B * heads * S, S, device=DEV)
    if drop:
        L.check(lib.kzv_debug_attn_dropout_mask(key, drop, B * heads, S, S, mask.data_ptr(), _st()), "mask")
    x = qkv.float().view(B, S, 3, heads, D).permute(2, 0, 3, 1, 4).clone().requires_grad_(True)      # [3, B, h, S, D]
    sc = (x[0] @ x[1].transpose(-1, -2)) * D ** -0.5
    pm = torch.softmax(sc, -1) * mask.view(B, heads, S, S)
    out = pm @ x[2]
    out.backward(dO.float().view(B, S, heads, D).permute(0, 2, 1, 3))
    want_o = out.detach().permute(0, 2, 1, 3).reshape(B * S, H)
    assert (O.float() - want_o).abs().max().item() < 2e-2 * want_o.abs().max().item() + 2e-3
    assert (lse - torch.logsumexp(sc.detach(), -1)).abs().max().item() < 1e-3
    want_g = x.grad.permute(1, 3, 0, 2, 4).reshape(B * S, 3 * H)
    err = (dqkv.float() - want_g).abs().max().item()
    assert err < 3e-2 * want_g.abs().max().item() + 2e-3, err


@pytest.mark.parametrize("B,nb,V", [(1, 1, 41), (5, 2, 157), (7, 3, 1000), (256, 4, 4300), (3, 8, 4300)])
def test_beam_topk_matches_log_softmax_plus_topk(lib, B, nb, V):
    """kzv_beam_topk against the torch expression it replaces in kzv/beam.py (log_softmax + beam score, top 2 * nb of the
    nb * V continuations per image, best first); with a padded row stride, dead beams (score -1e9) and exact ties."""
    torch.manual_seed(B * V + nb)
    K, ld = 2 * nb, V + 4
    buf = torch.randn(B * nb, ld, device=DEV) * 3
    logits = buf[:, :V]
    sc = torch.randn(B, nb, device=DEV)
    sc[0, 1:] = -1.0e9                                    # first step of a generation: only beam 0 is live
    out_lp = torch.empty(B, K, device=DEV)
    out_ix = torch.empty(B, K, dtype=torch.int64, device=DEV)
    L.check(lib.kzv_beam_topk(logits.data_ptr(), ld, sc.data_ptr(), B, nb, V, K, out_lp.data_ptr(), out_ix.data_ptr(), _st()), "beam_topk")
    torch.cuda.synchronize()
    acc = (torch.log_softmax(logits.float(), dim=-1).view(B, nb, V) + sc.unsqueeze(-1)).view(B, nb * V)
    ref_lp, ref_ix = acc.topk(K, dim=1)
    assert torch.equal(out_ix, ref_ix)
    assert (out_lp - ref_lp).abs().max().item() < 2e-5 * max(1.0, ref_lp[ref_lp > -1e8].abs().max().item())
    # ties: identical rows with identical scores -> the smaller flat index (beam * V + token) first
    if nb > 1:
        buf[:nb] = buf[0]
        sc[0] = 0.25
        L.check(lib.kzv_beam_topk(logits.data_ptr(), ld, sc.data_ptr(), B, nb, V, K, out_lp.data_ptr(), out_ix.data_ptr(), _st()), "beam_topk")
        torch.cuda.synchronize()
        best = int(logits[0].argmax())
        assert out_ix[0, :nb].tolist() == [k * V + best for k in range(nb)]
        assert float(out_lp[0, 0]) == float(out_lp[0, nb - 1])
    assert lib.kzv_beam_topk(logits.data_ptr(), ld, sc.data_ptr(), B, 9, V, 16, out_lp.data_ptr(), out_ix.data_ptr(), _st()) != 0      # > 8 beams


@pytest.mark.parametrize("M,N,K,epi,which", [(1, 256, 256, 0, "a"), (100, 768, 256, 0, "a"), (256, 768, 256, 2, "a"), (37, 256, 256, 5, "a"),
                                              (1024, 4300, 256, 1, "a"), (256, 256, 256, 3, "r"), (1000, 256, 768, 3, "r"), (5, 256, 1024, 3, "r")])
def test_gemm_rows_with_folded_layernorm(lib, M, N, K, epi, which):
    """kzv_gemm_rows_ln (generation step, hidden 256): A = LN(x) or residual = LN(x) computed inside the GEMM, against
    kzv_layernorm_fwd followed by kzv_gemm_nt on the few-rows kernel (summation order differs: a bf16 step here and there)."""
    torch.manual_seed(M + N + K + epi)
    x = torch.randn(M, 256, device=DEV) * 2 + 0.3
    gamma = torch.randn(256, device=DEV)
    beta = torch.randn(256, device=DEV)
    B = (torch.randn(N, K, device=DEV) * 0.1).bfloat16()
    bias = torch.randn(N, device=DEV)
    y16 = torch.empty(M, 256, dtype=torch.bfloat16, device=DEV)
    y32 = torch.empty(M, 256, device=DEV)
    L.check(lib.kzv_layernorm_fwd(x.data_ptr(), gamma.data_ptr(), beta.data_ptr(), y16.data_ptr(), y32.data_ptr(), None, M, 256, 1e-12, _st()), "ln")
    f32out = epi in (L.EPI_F32, L.EPI_RESID, 5)
    out = torch.empty(M, N, dtype=torch.float32 if f32out else torch.bfloat16, device=DEV)
    aux = torch.empty(M, N, dtype=torch.bfloat16, device=DEV) if epi in (2, 5) else None
    aux2 = torch.empty_like(aux) if aux is not None else None
    L.check(lib.kzv_set_rows_max_m(4096), "rows_max_m")
    try:
        if which == "a":
            ref = _gemm_nt(lib, y16, B, epi, bias, aux=aux)
            a = L.kzv_gemm_rows_ln_args(A=None, lda=0, B=B.data_ptr(), ldb=K, C=out.data_ptr(), ldc=N, bias=bias.data_ptr(), aux=L.ptr(aux2), ldaux=N,
                                        M=M, N=N, K=K, n_valid=N, ln_a=x.data_ptr(), ln_a_gamma=gamma.data_ptr(), ln_a_beta=beta.data_ptr(), eps=1e-12)
        else:
            A = torch.randn(M, K, device=DEV).bfloat16()
            ref = _gemm_nt(lib, A, B, epi, bias, resid=y32)
            a = L.kzv_gemm_rows_ln_args(A=A.data_ptr(), lda=K, B=B.data_ptr(), ldb=K, C=out.data_ptr(), ldc=N, bias=bias.data_ptr(), M=M, N=N, K=K, n_valid=N,
                                        ln_r=x.data_ptr(), ln_r_gamma=gamma.data_ptr(), ln_r_beta=beta.data_ptr(), eps=1e-12)
        L.check(lib.kzv_gemm_rows_ln(C.byref(a), epi, _st()), "gemm_rows_ln")
    finally:
        L.check(lib.kzv_set_rows_max_m(0), "rows_max_m")
    torch.cuda.synchronize()
    scale = max(1.0, ref.float().abs().max().item())
    tol = (2e-5 if which == "r" else 3e-3) * scale + (0 if f32out else 2 ** -8 * scale)
    assert (out.float() - ref.float()).abs().max().item() < tol
    if aux is not None:
        assert (aux2.float() - aux.float()).abs().max().item() < 2e-2
    bad = L.kzv_gemm_rows_ln_args(A=None, lda=0, B=B.data_ptr(), ldb=K, C=out.data_ptr(), ldc=N, M=M, N=N, K=K, n_valid=N)
    assert lib.kzv_gemm_rows_ln(C.byref(bad), epi, _st()) != 0          # nothing to normalise and no A
