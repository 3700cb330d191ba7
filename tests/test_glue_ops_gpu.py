"""Per-op references for the glue kernels (csrc/elementwise.hip; cross-entropy: csrc/cross_entropy.hip), LayerNorm in every instantiation and fused form
(csrc/layernorm.hip) and the hidden-state dropout generator every fused epilogue draws from, through the per-op C ABI.

The whole-step parity tests bound logits by 3e-2 and gradients by a few percent of their largest entry; a fault confined to part
of a tensor -- a mask indexed wrongly in a ragged last block, a CLS-row remap off at image boundaries, a bias gradient missing one
workgroup's share, padded columns leaking into a cross-entropy row -- vanishes inside those bounds.  Here every kernel is compared
on its own with a float64 torch statement of the same operation on the same (bf16-rounded) inputs, at sizes of a few workgroups:
odd sizes, ragged last blocks, and every size at which a launcher picks another kernel.

  * masks come from oracle/hidden_dropout.py (numpy); kzv_debug_dropout_mask is pinned to it bit for bit first, and serves as the
    mask of the larger shapes afterwards;
  * outputs a kernel overwrites are NaN-filled before the call; outputs it accumulates into start from a random base;
  * every mask and remap comparison proves it can fail (the idiom of tests/test_bench_geometry_gpu.py): the same comparison is
    run against a deliberately wrong reference -- the mask of key + 1, the mask indexed with ld_index + 4, the CLS remap without
    its "- 1" -- and must reject it (_must_reject);
  * accumulated sums (bias / embedding gradients) are judged per entry against 4e-6 of the entry's sum of |terms| (_acc_check): a
    few fp32 roundings of partial sums, where one missing term or workgroup share is >= 1e-3 of that sum at these sizes.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from kzv import _lib as L
from oracle import hidden_dropout as HD

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAN = float("nan")
LN_EPS = 1e-12
BF16_HALF_ULP = 2 ** -8      # |bf16(x) - x| <= 2^-8 |x| (8 significand bits, round to nearest even)


@pytest.fixture(scope="module")
def lib():
    return L.load()


def _st():
    return torch.cuda.current_stream().cuda_stream


def _gen(seed):
    return torch.Generator(device=DEV).manual_seed(seed)


def _randn(g, *shape):
    return torch.randn(*shape, device=DEV, generator=g)


def _nan(*shape, dtype=torch.float32):
    return torch.full(shape, NAN, dtype=dtype, device=DEV)


def _mask(lib, key, p, rows, cols, ld=None):
    """kzv_debug_dropout_mask (pinned to the numpy statement by the first test of this file): fp32 [rows, cols] on the device."""
    out = _nan(rows, cols)
    L.check(lib.kzv_debug_dropout_mask(key, p, rows, cols, cols if ld is None else ld, out.data_ptr(), _st()), "debug_dropout_mask")
    return out


def _must_reject(check, *wrong_refs):
    """The self-check every mask / remap comparison owes: ``check(reference)`` asserts; it must raise for each wrong reference."""
    for i, wrong in enumerate(wrong_refs):
        with pytest.raises(AssertionError):
            check(wrong)
            pytest.fail(f"the comparison accepted wrong reference #{i}", pytrace=False)


def _wrong_masks(lib, key, p, rows, cols, ld=None):
    """The two wrong masks of the self-check: another key, and the right key indexed with a row stride 4 too long (row 0 of that
    one is the right mask's row 0, so a single row gets the first only)."""
    ld = cols if ld is None else ld
    other_key = _mask(lib, key + 1, p, rows, cols, ld)
    return (other_key,) if rows == 1 else (other_key, _mask(lib, key, p, rows, cols, ld + 4))


def _err(got, want):
    """|got - want| in float64; a NaN on one side only (an unwritten or a wrongly written element) counts as inf."""
    g, w = got.double(), want.double()
    d = (g - w).abs()
    d[torch.isnan(g) & torch.isnan(w)] = 0.0
    return torch.nan_to_num(d, nan=float("inf"))


def _within(name, err, tol):
    bad = ~(err <= tol)
    if bool(bad.any()):
        i = bad.nonzero()[0].tolist()
        raise AssertionError(f"{name}: {int(bad.sum())} of {bad.numel()} outside the bound, first at {i}: error "
                             f"{float(err[tuple(i)]):.4g}, bound {float(tol[tuple(i)] if torch.is_tensor(tol) and tol.dim() else tol):.4g}")
    ratio = err / tol
    return float(torch.nan_to_num(ratio, nan=0.0).max())


def _acc_check(name, got, base, terms_sum, terms_abs):
    """An output a kernel ACCUMULATES into: got = base + sum(terms), in fp32 in some order.  Bound per entry: 4e-6 of the sum of
    the absolute values of everything the entry adds up, the base included.  The base is there because these kernels add INTO it,
    most of them with one float atomic per workgroup or per token row: each of those k adds rounds a running value of up to
    |base| + sum |terms|, an error of up to k 2^-24 (|base| + sum |terms|) that no multiple of sum |terms| alone bounds when the
    terms are few, small or cancel (M = 1; an id drawn twice with small gradients; all but one of three samples dropped).  k is
    at most ~40 here (embed_scatter_bwd, 200 rows on 12 ids): 2.4e-6."""
    want = base.double() + terms_sum
    tol = 4e-6 * (base.double().abs() + terms_abs)
    return _within(name, _err(got, want), tol)


# ================================================================================================ the mask generator
@pytest.mark.parametrize("p", [0.1, 0.3, 0.0])
@pytest.mark.parametrize("rows,cols,ld", [(7, 12, 12), (333, 768, 768), (64, 100, 260)])
def test_hidden_dropout_mask_entry_equals_the_numpy_statement(lib, rows, cols, ld, p):
    """kzv_debug_dropout_mask, which every replay test trusts, bit for bit against oracle/hidden_dropout.py."""
    for key in (0, 0xdeadbeef, 12345):
        got = _mask(lib, key, p, rows, cols, ld).cpu().numpy()

        def check(want):
            assert np.array_equal(got, want), key
        check(HD.multiplier(key, p, rows, cols, ld))
        if p > 0:
            _must_reject(check, HD.multiplier((key + 1) & 0xFFFFFFFF, p, rows, cols, ld), HD.multiplier(key, p, rows, cols, ld + 4))


# ================================================================================================ GEMM residual dropout
def _gemm_mask_case(lib, M, N, K, nv, ldc=None):
    """A = 0, B = 0, bias = 1, resid = 0, EPI_RESID, p = 0.1: the output IS the multiplier of element m * N + n."""
    key, p = 4242 + M + K, 0.1
    ldc = ldc or N
    A = torch.zeros(M, K, dtype=torch.bfloat16, device=DEV)
    B = torch.zeros(nv, K, dtype=torch.bfloat16, device=DEV)
    bias = torch.ones(nv, device=DEV)
    res = torch.zeros(M, ldc, device=DEV)
    out = _nan(M, ldc)
    a = L.kzv_gemm_nt_args(A=A.data_ptr(), lda=K, B=B.data_ptr(), ldb=K, C=out.data_ptr(), ldc=ldc, bias=bias.data_ptr(),
                           resid=res.data_ptr(), ldr=ldc, aux=None, ldaux=ldc, M=M, N=N, K=K, n_valid=nv, drop_p=p, drop_key=key)
    L.check(lib.kzv_gemm_nt(C.byref(a), L.EPI_RESID, _st()), "gemm_nt")
    got = out[:, :nv]

    def check(mask):
        assert torch.equal(got, mask[:, :nv])
    check(_mask(lib, key, p, M, N))
    _must_reject(check, *_wrong_masks(lib, key, p, M, N))
    frac = float((got == 0).float().mean())
    assert 0.08 < frac < 0.12, frac          # the mask is a mask (not all ones / all zeros): >= 26k samples, sigma <= 0.002


BIG = (24600, 1024)        # >= 384 tiles of 256 x 256 (tests/test_ops_gpu.py: the shapes that reach the 256x256 kernels)


@pytest.mark.parametrize("family,M,N,K,nv,ldc", [
    ("few-rows", 200, 132, 128, 132, None),
    ("128x128", 483, 384, 192, 384, None),
    ("128x128", 130, 192, 64, 157, None),
    ("128x128 ldc>N", 483, 384, 192, 384, 392),
    ("persistent 256x256", *BIG, 128, 1000, None),
    ("one-tile 256x256", *BIG, 320, 1000, None),
    ("free-running", *BIG, 256, 1000, None),
    ("four-wave", *BIG, 384, 1000, None),
])
def test_gemm_residual_dropout_draws_the_debug_mask_in_every_kernel_family(lib, family, M, N, K, nv, ldc):
    """The RESID epilogue of every kzv_gemm_nt kernel family (knobs and shapes as tests/test_ops_gpu.py documents them) draws
    exactly kzv_debug_dropout_mask(key, p, M, N, ld_index = N): ragged M, n_valid < N (columns >= n_valid are not compared), and
    one case with ldc = N + 8 -- the index follows N, not the stride (gemm_nt.h nt_emit).  Which kernel ran is not verified at run
    time: the family follows from kzv_gemm_nt's dispatch conditions (csrc/gemm.hip) at these knobs and shapes."""
    try:
        if family == "few-rows":
            L.check(lib.kzv_set_rows_max_m(1024), "rows_max_m")
        elif family == "free-running":
            L.check(lib.kzv_set_nt_schedule(1), "nt_schedule")
        elif family == "four-wave":
            L.check(lib.kzv_set_nt_schedule(2), "nt_schedule")
        _gemm_mask_case(lib, M, N, K, nv, ldc)
    finally:
        L.check(lib.kzv_set_rows_max_m(0), "rows_max_m")
        L.check(lib.kzv_set_nt_schedule(-1), "nt_schedule")


# ================================================================================================ LayerNorm
def _ln_inputs(rows, H, seed):
    g = _gen(seed)
    x = _randn(g, rows, H) * 2 + 0.5
    gamma = 1 + 0.1 * _randn(g, H)
    beta = 0.1 * _randn(g, H)
    return x, gamma, beta, g


def _ln_fwd_ref(x, gamma, beta):
    xd = x.double()
    mean = xd.mean(1, keepdim=True)
    rstd = (xd.var(1, unbiased=False, keepdim=True) + LN_EPS).rsqrt()
    xhat = (xd - mean) * rstd
    return {"y": xhat * gamma.double() + beta.double(), "mean": mean[:, 0], "rstd": rstd[:, 0], "xhat": xhat,
            "xmax": xd.abs().amax(1)}


def _ln_bwd_ref(ref, gamma, d):
    """float64 LayerNorm backward of dy = d ([rows, H], already masked / remapped / rounded by the caller)."""
    d = d.double()
    xhat, rstd = ref["xhat"], ref["rstd"][:, None]
    gy = d * gamma.double()
    m1, m2 = gy.mean(1, keepdim=True), (gy * xhat).mean(1, keepdim=True)
    return {"dx": rstd * (gy - m1 - xhat * m2), "dg": (d * xhat).sum(0), "db": d.sum(0),
            "sg": (d * xhat).abs().sum(0), "sb": d.abs().sum(0)}


def _ln_fwd(lib, x, gamma, beta, out_rows=None, seq=1, drop_first=0, p=0.0, key=0):
    rows, H = x.shape
    n = rows if out_rows is None else out_rows
    y16, y32, stats = _nan(n, H, dtype=torch.bfloat16), _nan(n, H), _nan(rows, 2)
    a = L.kzv_ln_fwd_args(x=x.data_ptr(), gamma=gamma.data_ptr(), beta=beta.data_ptr(), y_bf16=y16.data_ptr(), y_f32=y32.data_ptr(),
                          stats=stats.data_ptr(), rows=rows, H=H, seq=seq, drop_first=drop_first, eps=LN_EPS, drop_p=p, drop_key=key)
    L.check(lib.kzv_ln_fwd_ex(C.byref(a), _st()), "ln_fwd_ex")
    return y16, y32, stats


def _ln_bwd(lib, dy, x, stats, gamma, gen, accumulate, seq=1, drop_first=0, p=0.0, key=0, want_out16=False, out_p=0.0, out_key=0):
    """Runs kzv_ln_bwd_ex; dx starts from a random base (accumulate) or NaN, dgamma / dbeta from random bases.  Returns the
    buffers after the call and the bases."""
    rows, H = x.shape
    dx0 = _randn(gen, rows, H) if accumulate else _nan(rows, H)
    dg0, db0 = _randn(gen, H), _randn(gen, H)
    dx, dg, db = dx0.clone(), dg0.clone(), db0.clone()
    out16 = _nan(rows, H, dtype=torch.bfloat16) if want_out16 else None
    a = L.kzv_ln_bwd_args(dy=dy.data_ptr(), x=x.data_ptr(), stats=stats.data_ptr(), gamma=gamma.data_ptr(), dx=dx.data_ptr(),
                          dgamma=dg.data_ptr(), dbeta=db.data_ptr(), out16=L.ptr(out16), dy_is_f32=int(dy.dtype == torch.float32),
                          accumulate_dx=int(accumulate), rows=rows, H=H, seq=seq, drop_first=drop_first, drop_p=p, drop_key=key,
                          out_drop_p=out_p, out_drop_key=out_key)
    L.check(lib.kzv_ln_bwd_ex(C.byref(a), _st()), "ln_bwd_ex")
    return {"dx": dx, "dg": dg, "db": db, "out16": out16, "dx0": dx0, "dg0": dg0, "db0": db0, "acc": accumulate}


def _ln_check_fwd(tag, y16, y32, want_y):
    """y (fp32) within 2e-5, y (bf16) within 2^-8 of the row's largest |y| (tests/test_bench_geometry_gpu.py _ln_compare); rows the
    reference holds as NaN must be NaN (never written)."""
    rowmax = torch.nan_to_num(want_y, nan=0.0).abs().amax(1, keepdim=True)
    _within(f"{tag} y32", _err(y32, want_y), torch.full_like(want_y, 2e-5))
    _within(f"{tag} y16", _err(y16, want_y), ((BF16_HALF_ULP + 1e-6) * rowmax).expand_as(want_y))


def _ln_check_stats(tag, stats, ref):
    _within(f"{tag} mean", _err(stats[:, 0], ref["mean"]), 1e-5 * ref["xmax"])
    _within(f"{tag} rstd", _err(stats[:, 1], ref["rstd"]), 1e-5 * ref["rstd"])


def _ln_check_bwd(tag, got, want):
    """dx per row within 3e-5 max(1, the row's largest |dx|); dgamma / dbeta (less their bases) per column within 4e-6 of the
    column's sum of |terms| (test_layernorm_fwd_bwd / _ln_compare)."""
    dx = got["dx"].double() - got["dx0"].double() if got["acc"] else got["dx"]
    _within(f"{tag} dx", _err(dx, want["dx"]), (3e-5 * want["dx"].abs().amax(1, keepdim=True).clamp(min=1.0)).expand_as(want["dx"]))
    _within(f"{tag} dgamma", _err(got["dg"].double() - got["dg0"].double(), want["dg"]), 4e-6 * want["sg"])
    _within(f"{tag} dbeta", _err(got["db"].double() - got["db0"].double(), want["db"]), 4e-6 * want["sb"])


@pytest.mark.parametrize("rows", [7, 333])
@pytest.mark.parametrize("H", [64, 256, 384, 512, 640, 768, 900, 1024, 1284, 2048])
def test_layernorm_every_instantiation(lib, rows, H):
    """Forward NC = 1 (H 64, 256), 2 (384, 512), 3 (640, 768), 4 (900, 1024), 8 (1284, 2048); backward: the pipelined kernel for
    H = 256 k <= 1024 in its four (dy type, accumulate) instantiations, the generic kernel for every other H (NC 1, 2, 3, 4, 8).
    7 rows: one ragged forward workgroup and backward wave; 333: six 64-row backward workgroups, the last with 13 rows."""
    x, gamma, beta, g = _ln_inputs(rows, H, 1000 * rows + H)
    ref = _ln_fwd_ref(x, gamma, beta)
    y16, y32, stats = _ln_fwd(lib, x, gamma, beta)
    _ln_check_fwd(f"ln {rows}x{H}", y16, y32, ref["y"])
    _ln_check_stats(f"ln {rows}x{H}", stats, ref)
    dy = _randn(g, rows, H)
    for dy_in in (dy, dy.bfloat16()):
        want = _ln_bwd_ref(ref, gamma, dy_in)
        for acc in (0, 1):
            got = _ln_bwd(lib, dy_in, x, stats, gamma, g, acc)
            _ln_check_bwd(f"ln {rows}x{H} bwd dy {dy_in.dtype} acc {acc}", got, want)


FUSED_H = [256, 768, 384]      # pipelined backward NC 1 and 3, generic backward NC 2


@pytest.mark.parametrize("seq,images", [(5, 27), (161, 3)])
@pytest.mark.parametrize("H", FUSED_H)
def test_layernorm_drop_first_remaps_rows_and_skips_cls(lib, H, seq, images):
    """seq / drop_first (the encoder's final LayerNorm drops CLS): output row r - r / seq - 1, CLS rows write nothing (exactly
    (seq - 1) * images rows of the NaN-filled outputs are written, the first ones), statistics for ALL rows; backward reads dy at
    the remapped row, CLS rows get the LayerNorm backward of a zero dy (0, or the accumulated base untouched), dgamma / dbeta
    exclude them.  27 x 5: image boundaries inside every 64-row backward workgroup; 3 x 161: the bench's sequence length."""
    rows, n_out = seq * images, (seq - 1) * images
    x, gamma, beta, g = _ln_inputs(rows, H, 77 * seq + H)
    ref = _ln_fwd_ref(x, gamma, beta)
    r = torch.arange(rows, device=DEV)
    is_cls = r % seq == 0
    right, wrong = r - r // seq - 1, r - r // seq                      # the remap, and the remap without its "- 1"

    y16, y32, stats = _ln_fwd(lib, x, gamma, beta, out_rows=rows, seq=seq, drop_first=1)
    _ln_check_stats(f"ln drop_first {seq}x{images} H {H}", stats, ref)
    for y in (y16, y32):
        written = ~torch.isnan(y.float()).all(1)
        assert int(written.sum()) == n_out and bool(written[:n_out].all()), int(written.sum())

    def check_fwd(remap):
        want = _nan(rows, H, dtype=torch.float64)
        want[remap[~is_cls]] = ref["y"][~is_cls]
        _ln_check_fwd(f"ln drop_first {seq}x{images} H {H}", y16, y32, want)
    check_fwd(right)
    _must_reject(check_fwd, wrong)

    dy = _randn(g, n_out, H)
    for dy_in, acc in ((dy, 0), (dy.bfloat16(), 1)):
        got = _ln_bwd(lib, dy_in, x, stats, gamma, g, acc, seq=seq, drop_first=1)
        cls_dx = got["dx"][is_cls]
        assert torch.equal(cls_dx, got["dx0"][is_cls] if acc else torch.zeros_like(cls_dx))

        def check_bwd(remap):
            d = dy_in.double()[remap.clamp(max=n_out - 1)]
            d[is_cls] = 0.0
            _ln_check_bwd(f"ln drop_first {seq}x{images} H {H} bwd acc {acc}", got, _ln_bwd_ref(ref, gamma, d))
        check_bwd(right)
        _must_reject(check_bwd, wrong)


@pytest.mark.parametrize("H", FUSED_H)
def test_layernorm_forward_dropout_draws_the_mask_of_the_output_index(lib, H):
    rows, p, key = 333, 0.1, 900 + H
    x, gamma, beta, _ = _ln_inputs(rows, H, 31 + H)
    ref = _ln_fwd_ref(x, gamma, beta)
    assert bool((ref["y"] != 0).all())                  # so that an output is zero iff it was dropped
    y16, y32, _ = _ln_fwd(lib, x, gamma, beta, p=p, key=key)

    def check(mask):
        assert torch.equal(y32 == 0, mask == 0) and torch.equal(y16 == 0, mask == 0)
        _ln_check_fwd(f"ln fwd dropout H {H}", y16, y32, ref["y"] * mask.double())
    check(_mask(lib, key, p, rows, H))
    _must_reject(check, *_wrong_masks(lib, key, p, rows, H))


@pytest.mark.parametrize("H", FUSED_H)
def test_layernorm_backward_dropout_masks_dy(lib, H):
    """drop_p / drop_key of the backward: dy is masked first (the LayerNorm behind a dropout).  Reference: the float64 backward of
    dy * mask; one wrong mask bit moves a dx row by ~|dy| and its column of dbeta by |dy| / 0.9."""
    rows, p, key = 333, 0.1, 1700 + H
    x, gamma, beta, g = _ln_inputs(rows, H, 57 + H)
    ref = _ln_fwd_ref(x, gamma, beta)
    _, _, stats = _ln_fwd(lib, x, gamma, beta)
    dy = _randn(g, rows, H)
    for dy_in, acc in ((dy, 1), (dy.bfloat16(), 0)):
        got = _ln_bwd(lib, dy_in, x, stats, gamma, g, acc, p=p, key=key)

        def check(mask):
            _ln_check_bwd(f"ln bwd dropout H {H} acc {acc}", got, _ln_bwd_ref(ref, gamma, dy_in.double() * mask.double()))
        check(_mask(lib, key, p, rows, H))
        _must_reject(check, *_wrong_masks(lib, key, p, rows, H))


@pytest.mark.parametrize("out_p", [0.0, 0.1])
@pytest.mark.parametrize("acc", [0, 1])
@pytest.mark.parametrize("H", FUSED_H)
def test_layernorm_backward_out16_is_the_masked_bf16_copy_of_the_stored_dx(lib, H, acc, out_p):
    """out16 = bf16(dx_written * mask) bit for bit, dx_written = the fp32 dx row this call stored (the TOTAL under accumulate_dx);
    the mask is indexed by the LayerNorm row (row * H + col), the index of the cast + column-sum kernel it replaces."""
    rows, key = 333, 2600 + H
    x, gamma, beta, g = _ln_inputs(rows, H, 91 + H)
    ref = _ln_fwd_ref(x, gamma, beta)
    _, _, stats = _ln_fwd(lib, x, gamma, beta)
    dy = _randn(g, rows, H).bfloat16()
    got = _ln_bwd(lib, dy, x, stats, gamma, g, acc, want_out16=True, out_p=out_p, out_key=key)
    _ln_check_bwd(f"ln out16 H {H} acc {acc}", got, _ln_bwd_ref(ref, gamma, dy))

    def check(mask):
        assert torch.equal(got["out16"], (got["dx"] * mask).bfloat16())
    check(_mask(lib, key, out_p, rows, H))
    if out_p > 0:
        _must_reject(check, *_wrong_masks(lib, key, out_p, rows, H))


# ================================================================================================ embedding assembly
def _pos_rows(np_, gw, gw_max):
    """Position-table row of every token (0 = CLS): patch p of a gw-wide grid sits at (p / gw, p % gw) of the gw_max-wide table."""
    pch = torch.arange(np_, device=DEV)
    return torch.cat([torch.zeros(1, dtype=torch.long, device=DEV), 1 + (pch // gw) * gw_max + pch % gw])


EMBED_GRIDS = [(10, 5, 5, 11), (6, 3, 5, 11)]        # (np, gw, gw_max, position-table rows)


@pytest.mark.parametrize("np_,gw,gw_max,table", EMBED_GRIDS)
@pytest.mark.parametrize("He", [64, 132])
@pytest.mark.parametrize("B", [3, 70])
def test_embed_assemble_forward(lib, B, He, np_, gw, gw_max, table):
    S = np_ + 1
    g = _gen(B * 1000 + He + np_)
    pe, cls, pos = _randn(g, B, np_, He), _randn(g, He), _randn(g, table, He)
    x0 = _nan(B, S, He)
    L.check(lib.kzv_embed_assemble(pe.data_ptr(), cls.data_ptr(), pos.data_ptr(), x0.data_ptr(), B, np_, He, 0.0, 0, gw, gw_max, _st()), "embed_assemble")
    want = torch.cat([cls.expand(B, 1, He), pe], 1) + pos[_pos_rows(np_, gw, gw_max)]
    assert torch.equal(x0, want)                                      # one fp32 add: exact
    # dropout: cat(cls, patches) + pos == 1 everywhere -> the output IS the multiplier of element row * He + col
    key, p = 555 + B + He, 0.1
    x0.fill_(NAN)
    pe.fill_(1.0); cls.fill_(1.0); pos.zero_()
    L.check(lib.kzv_embed_assemble(pe.data_ptr(), cls.data_ptr(), pos.data_ptr(), x0.data_ptr(), B, np_, He, p, key, gw, gw_max, _st()), "embed_assemble")

    def check(mask):
        assert torch.equal(x0.view(B * S, He), mask)
    check(_mask(lib, key, p, B * S, He))
    _must_reject(check, *_wrong_masks(lib, key, p, B * S, He))


@pytest.mark.parametrize("np_,gw,gw_max,table", EMBED_GRIDS)
@pytest.mark.parametrize("He", [64, 132])
@pytest.mark.parametrize("B", [3, 70])
def test_embed_assemble_backward(lib, B, He, np_, gw, gw_max, table):
    """B = 3: one batch chunk of 32; B = 70: three chunks, the last of 6.  dpatch bit for bit; dcls / dpos / patch-bias gradient
    accumulated into random bases against float64; position rows no token maps to keep their base exactly; two runs are
    bit-identical (the sums have a fixed order, no atomics)."""
    S = np_ + 1
    key, p = 808 + B + He, 0.1
    g = _gen(B * 77 + He + np_)
    dx0 = _randn(g, B, S, He)
    bases = [_randn(g, He), _randn(g, table, He), _randn(g, He)]        # dcls, dpos, dpatch_bias
    prow = _pos_rows(np_, gw, gw_max)

    def run():
        dpatch = _nan(B, np_, He, dtype=torch.bfloat16)
        dcls, dpos, dpb = (t.clone() for t in bases)
        L.check(lib.kzv_embed_assemble_bwd(dx0.data_ptr(), dpatch.data_ptr(), dcls.data_ptr(), dpos.data_ptr(), dpb.data_ptr(), B, np_, He,
                                           p, key, gw, gw_max, _st()), "embed_assemble_bwd")
        return dpatch, dcls, dpos, dpb
    dpatch, dcls, dpos, dpb = run()
    for a, b in zip(run(), (dpatch, dcls, dpos, dpb)):
        assert torch.equal(a, b)
    untouched = torch.ones(table, dtype=torch.bool, device=DEV)
    untouched[prow] = False
    assert int(untouched.sum()) == table - S
    assert torch.equal(dpos[untouched], bases[1][untouched])

    def check(mask):
        masked = dx0 * mask.view(B, S, He)                              # fp32, as the kernel multiplies
        assert torch.equal(dpatch, masked[:, 1:].bfloat16())
        tok, tok_abs = masked.double().sum(0), masked.double().abs().sum(0)          # [S, He]
        tag = f"embed_assemble_bwd B {B} He {He} np {np_}"
        _acc_check(f"{tag} dcls", dcls, bases[0], tok[0], tok_abs[0])
        _acc_check(f"{tag} dpos", dpos[prow], bases[1][prow], tok, tok_abs)
        _acc_check(f"{tag} dpatch_bias", dpb, bases[2], tok[1:].sum(0), tok_abs[1:].sum(0))
    check(_mask(lib, key, p, B * S, He))
    _must_reject(check, *_wrong_masks(lib, key, p, B * S, He))


# ================================================================================================ cast + dropout + column sums
@pytest.mark.parametrize("gelu", [False, True])
@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("N", [4, 256, 260, 768])
@pytest.mark.parametrize("M", [1, 70, 333])
def test_cast_drop_colsum(lib, M, N, p, gelu):
    """out = bf16((g * mask) * gelu') bit for bit (fp32 products in that order); dbias += the column sums of the ROUNDED out.
    M = 1 / 70 / 333: one row, a second (ragged) 64-row block, six blocks adding into one column with float atomics; N = 4 / 260:
    one lane, and a second column block of one lane."""
    key = 3000 + M + N
    gen = _gen(M * 1000 + N)
    g = _randn(gen, M, N)
    pre = (torch.rand(M, N, device=DEV, generator=gen) * 1.26 - 0.13).bfloat16() if gelu else None
    base = _randn(gen, N)
    out, dbias = _nan(M, N, dtype=torch.bfloat16), base.clone()
    L.check(lib.kzv_cast_drop_colsum(g.data_ptr(), out.data_ptr(), dbias.data_ptr(), M, N, p, key, L.ptr(pre), _st()), "cast_drop_colsum")

    def check(mask):
        v = g * mask
        if gelu:
            v = v * pre.float()
        want = v.bfloat16()
        assert torch.equal(out, want)
        _acc_check(f"cast_drop_colsum {M}x{N} dbias", dbias, base, want.double().sum(0), want.double().abs().sum(0))
    check(_mask(lib, key, p, M, N))
    if p > 0 and M * N >= 64:           # 1 x 4: four mask bits, a wrong key may draw the same ones
        _must_reject(check, *_wrong_masks(lib, key, p, M, N))


@pytest.mark.parametrize("N", [4, 256, 260, 768])
@pytest.mark.parametrize("M", [1, 70, 333])
def test_colsum_bf16_on_a_column_slice(lib, M, N):
    """colsum_kernel<false> with ld > N: the slice [32, 32 + N) of a [M, N + 64] buffer whose other columns hold NaN -- nothing
    outside the slice may reach the sums."""
    gen = _gen(M * 31 + N)
    ld = N + 64
    buf = _nan(M, ld, dtype=torch.bfloat16)
    gsl = buf[:, 32:32 + N]
    gsl.copy_(_randn(gen, M, N))
    base = _randn(gen, N)
    dbias = base.clone()
    L.check(lib.kzv_colsum_bf16(gsl.data_ptr(), ld, dbias.data_ptr(), M, N, _st()), "colsum_bf16")
    _acc_check(f"colsum_bf16 {M}x{N}", dbias, base, gsl.double().sum(0), gsl.double().abs().sum(0))


# ================================================================================================ decoder embeddings
PAD = 1


def _labels(B, L_, gen, vocab):
    """[B, L_] int64: BOS (0), a random number of characters >= 2 (repeated ids), EOS (2), padding; row 1 = BOS + padding only, row 2
    without padding."""
    lab = torch.randint(3, vocab, (B, L_), device=DEV, generator=gen, dtype=torch.int64)
    lab[:, 0] = 0
    n = torch.randint(2, L_ - 2, (B,), device=DEV, generator=gen)
    col = torch.arange(L_, device=DEV)[None]
    lab[col == (n[:, None] + 1)] = 2
    lab[col > (n[:, None] + 1)] = PAD
    if B > 1:
        lab[1, 1:] = PAD
    if B > 2:
        lab[2, 1:] = torch.randint(3, vocab, (L_ - 1,), device=DEV, generator=gen, dtype=torch.int64)
    return lab


def _posids_ref(lab, T):
    live = lab[:, :T] != PAD
    return (torch.cumsum(live, 1) * live + PAD).to(torch.int32)


@pytest.mark.parametrize("T", [11, 7])
def test_dec_prepare(lib, T):
    B, L_ = 5, 12
    lab = _labels(B, L_, _gen(T), 50)
    assert bool((lab[1, 1:] == PAD).all()) and bool((lab[2] != PAD).all())
    want = _posids_ref(lab, T)
    want_count = float((lab[:, 1:T + 1] != PAD).sum())
    for max_pos, overflow in ((40, False), (6, True)):
        posids = torch.full((B, T), -7, dtype=torch.int32, device=DEV)
        count, err = torch.zeros(1, device=DEV), torch.zeros(1, dtype=torch.int32, device=DEV)
        L.check(lib.kzv_dec_prepare(lab.data_ptr(), B, L_, T, PAD, max_pos, posids.data_ptr(), count.data_ptr(), err.data_ptr(), _st()), "dec_prepare")
        assert float(count) == want_count
        assert int(err) == int(overflow)
        assert bool((want >= max_pos).any()) == overflow              # the case does what its name says
        assert torch.equal(posids, want.clamp(max=max_pos - 1))


@pytest.mark.parametrize("Hd", [64, 256])
def test_embed_gather(lib, Hd):
    B, L_, T, V, max_pos = 5, 12, 11, 50, 40
    gen = _gen(Hd)
    lab = _labels(B, L_, gen, V)
    posids = _posids_ref(lab, T).contiguous()
    word, type0, postab = _randn(gen, V, Hd), _randn(gen, Hd), _randn(gen, max_pos, Hd)
    out = _nan(B * T, Hd)
    L.check(lib.kzv_embed_gather(lab.data_ptr(), L_, posids.data_ptr(), word.data_ptr(), type0.data_ptr(), postab.data_ptr(), out.data_ptr(),
                                 B, T, Hd, _st()), "embed_gather")
    ids = lab[:, :T].reshape(-1)
    want = (word[ids] + type0) + postab[posids.reshape(-1).long()]      # the kernel's association of its two fp32 adds
    assert torch.equal(out, want)


@pytest.mark.parametrize("Hd", [64, 256])
@pytest.mark.parametrize("B,T", [(3, 5), (7, 11), (8, 25)])
def test_embed_scatter_bwd(lib, B, T, Hd):
    """15 / 77 / 200 token rows (a partial 16-row wave; two workgroups; four), a 12-id vocabulary so that the float atomics collide
    on the same table rows; dword / dtype0 / dpostab accumulated into random bases against float64 index_add; the padding row of
    both tables keeps its base exactly."""
    L_, V, max_pos = T + 1, 12, T + 4
    gen = _gen(B * 100 + T + Hd)
    lab = _labels(B, L_, gen, V)
    posids = _posids_ref(lab, T).contiguous()
    dsum = _randn(gen, B * T, Hd)
    bases = [_randn(gen, V, Hd), _randn(gen, Hd), _randn(gen, max_pos, Hd)]
    dword, dtype0, dpostab = (t.clone() for t in bases)
    L.check(lib.kzv_embed_scatter_bwd(dsum.data_ptr(), lab.data_ptr(), L_, posids.data_ptr(), dword.data_ptr(), dtype0.data_ptr(), dpostab.data_ptr(),
                                      B, T, Hd, PAD, _st()), "embed_scatter_bwd")
    ids, pids, d = lab[:, :T].reshape(-1), posids.reshape(-1).long(), dsum.double()
    assert int((ids == PAD).sum()) > 0 and ids.unique().numel() < ids.numel()
    tag = f"embed_scatter_bwd {B}x{T} Hd {Hd}"
    for name, got, base, idx, rows in (("dword", dword, bases[0], ids, V), ("dpostab", dpostab, bases[2], pids, max_pos)):
        live = idx != PAD
        z = torch.zeros(rows, Hd, dtype=torch.float64, device=DEV)
        _acc_check(f"{tag} {name}", got, base, z.index_add(0, idx[live], d[live]), z.index_add(0, idx[live], d[live].abs()))
        assert torch.equal(got[PAD], base[PAD])
    _acc_check(f"{tag} dtype0", dtype0, bases[1], d.sum(0), d.abs().sum(0))


# ================================================================================================ cross entropy
# Loss bound: 4 x the worst |loss - float64 loss| measured over the six cases below on MI355X (both forms of the call).  The test
# prints every case's error before it asserts.  For scale: the losses are 10.5 .. 17.7, one fp32 ulp of 16 is 1.9e-6, and the
# rows' shares reach *loss by float atomics in no fixed order, so the last bit of the sum differs from call to call: the figure
# is the worst of two runs of the file (24 losses).
CE_LOSS_MEASURED = 1.93e-6         # V 4300, dlogits = NULL, one run of two (2.2e-8 in the other); every other loss <= 1.13e-6
CE_LOSS_BOUND = 4 * CE_LOSS_MEASURED


@pytest.mark.parametrize("V,ldl", [(41, 64), (777, 832), (4300, 4352), (5120, 5120), (5121, 5184), (6000, 6016)])
def test_cross_entropy_fwd_bwd(lib, V, ldl):
    """kzv_ce_fwd_bwd: ldl <= 5,120 takes ce_kernel (the row in registers), wider rows ce_generic_kernel (three passes).  B = 3,
    T = 7, label stride 16, logits randn * 4, padding columns [V, ldl) filled with +50 (a kernel that read them as logits would be
    far off), pad targets in three rows of image 0, all of image 1 and one of image 2.  dlogits: pad-target rows and columns
    [V, ldl) exactly zero, every other element within 2^-8 |want| + 1e-6 / count of the float64 (softmax - onehot) / count (one bf16
    rounding + the fp32 softmax); the dlogits = NULL form returns the same loss.

    Loss bound: the kernels use the fast exp / log, so the bound is measured, not derived.  Worst |loss - float64 loss| over these
    six cases on MI355X, both forms, two runs: 1.93e-6 (CE_LOSS_MEASURED; V 4300 without dlogits, one ulp of the loss 17.7; the
    same call was 2.2e-8 off in the other run, and every other loss within 1.13e-6); bound = 4 x that = 7.72e-6 (CE_LOSS_BOUND),
    four fp32 ulp of these losses.  The two forms run the same loss arithmetic and differ only in the order of the float atomics
    (by one ulp at most in these runs); each within the bound of float64 leaves them within eight ulp of each other."""
    B, T, L_ = 3, 7, 16
    gen = _gen(V)
    logits = _randn(gen, B * T, ldl) * 4
    logits[:, V:] = 50.0
    lab = torch.randint(2, V, (B, L_), device=DEV, generator=gen, dtype=torch.int64)
    lab[0, 5:] = PAD
    lab[1, :] = PAD
    lab[2, 7] = PAD
    tgt = lab[:, 1:T + 1].reshape(-1)
    live = tgt != PAD
    n = int(live.sum())
    assert 0 < n < B * T - T
    count = torch.tensor([float(n)], device=DEV)
    x = logits[:, :V].double()
    lse = torch.logsumexp(x, 1)
    safe = tgt.clamp(max=V - 1)
    want_loss = float(((lse - x.gather(1, safe[:, None])[:, 0]) * live).sum() / n)
    want = torch.zeros(B * T, ldl, dtype=torch.float64, device=DEV)
    want[:, :V] = (torch.softmax(x, 1) - torch.nn.functional.one_hot(safe, V)) / n
    want[~live] = 0.0

    losses = []
    for with_grad in (True, False):
        loss = torch.zeros(1, device=DEV)
        dl = _nan(B * T, ldl, dtype=torch.bfloat16) if with_grad else None
        L.check(lib.kzv_ce_fwd_bwd(logits.data_ptr(), ldl, lab.data_ptr(), L_, B, T, V, PAD, count.data_ptr(), loss.data_ptr(), L.ptr(dl), _st()), "ce_fwd_bwd")
        losses.append(float(loss))
        if with_grad:
            assert bool((dl[~live] == 0).all()) and bool((dl[:, V:] == 0).all())
            _within(f"ce V {V} dlogits", _err(dl, want), BF16_HALF_ULP * want.abs() + 1e-6 / n)
    errs = [abs(v - want_loss) for v in losses]
    print(f"ce V {V} ldl {ldl}: loss {losses[0]:.7f} (float64 {want_loss:.7f}), |error| {errs[0]:.3g} with dlogits, {errs[1]:.3g} without")
    assert max(errs) <= CE_LOSS_BOUND, (errs, CE_LOSS_BOUND)


# ================================================================================================ data movement, exact
@pytest.mark.parametrize("B,Cn,H,W,ph,pw", [(2, 3, 32, 64, 16, 16), (3, 1, 16, 48, 8, 16)])
def test_im2row(lib, B, Cn, H, W, ph, pw):
    px = _randn(_gen(H + W), B, Cn, H, W)
    gh, gw = H // ph, W // pw
    out = _nan(B * gh * gw, Cn * ph * pw, dtype=torch.bfloat16)
    L.check(lib.kzv_im2row(px.data_ptr(), out.data_ptr(), B, Cn, H, W, ph, pw, _st()), "im2row")
    want = px.bfloat16().view(B, Cn, gh, ph, gw, pw).permute(0, 2, 4, 1, 3, 5).reshape(B * gh * gw, Cn * ph * pw)
    assert torch.equal(out, want)
    unf = torch.nn.functional.unfold(px, (ph, pw), stride=(ph, pw)).transpose(1, 2).reshape(B * gh * gw, -1).bfloat16()
    assert torch.equal(want, unf)                                       # the reference is nn.Unfold's layout


def test_copy_logits(lib):
    gen = _gen(3)
    rows, V, Vp = 21, 41, 64
    buf = _randn(gen, rows, Vp)
    out = _nan(rows, V)
    L.check(lib.kzv_copy_logits(buf.data_ptr(), Vp, out.data_ptr(), rows, V, _st()), "copy_logits")
    assert torch.equal(out, buf[:, :V])
    # one position per image: row stride T * Vp from the row of position `pos`
    B, T, pos = 3, 7, 4
    buf = _randn(gen, B, T, Vp)
    out = _nan(B, V)
    L.check(lib.kzv_copy_logits(buf[0, pos].data_ptr(), T * Vp, out.data_ptr(), B, V, _st()), "copy_logits")
    assert torch.equal(out, buf[:, pos, :V])


def test_cast_weights_table_of_three(lib):
    """Three matrices in one descriptor table (2 + 12 + 1 tiles of 64 x 64: the kernel's binary search over tile0), the middle one
    with a transposed copy whose row stride (192) exceeds its 132 rows; every destination NaN-filled first."""
    gen = _gen(9)
    shapes = [(100, 64), (132, 256), (64, 64)]
    src = [_randn(gen, r, c) for r, c in shapes]
    dst = [_nan(r, c, dtype=torch.bfloat16) for r, c in shapes]
    ldT = 192
    dstT = _nan(256, ldT, dtype=torch.bfloat16)
    descs = (L.kzv_cast_desc * 3)()
    for i, (r, c) in enumerate(shapes):
        descs[i] = L.kzv_cast_desc(src=src[i].data_ptr(), dst=dst[i].data_ptr(), dstT=dstT.data_ptr() if i == 1 else None, rows=r, cols=c,
                                   ldT=ldT if i == 1 else 0)
    L.check(lib.kzv_cast_weights(descs, 3, _st()), "cast_weights")
    for s, d in zip(src, dst):
        assert torch.equal(d, s.bfloat16())
    assert torch.equal(dstT[:, :132], src[1].t().bfloat16())
    assert bool(torch.isnan(dstT[:, 132:].float()).all())               # the stride's slack is not written
    bad = (L.kzv_cast_desc * 1)(L.kzv_cast_desc(src=src[0].data_ptr(), dst=dst[0].data_ptr(), dstT=dstT.data_ptr(), rows=100, cols=64, ldT=64))
    assert lib.kzv_cast_weights(bad, 1, _st()) == -1                    # ldT < rows
