"""The hot kernels and the whole step at the BENCHMARK's launch geometry, against independent references.

bench.py times vit_b_config(dec_layers=6), init_seed=42, synthetic_batch(cfg, 256, 128, seed=1), dropout on: 256 x 161 =
41,216 encoder tokens, 3,072 encoder attention workgroups, a decoder trimmed to 60 positions.  The other tests run these
kernels at a few dozen workgroups; the bug class that slipped past them ("the >256-workgroup bug") was a stale
or early read that only shows when a launch has more workgroups than CUs.  Hence, for every comparison here:

  * each UNIT is judged on its own -- the part of the output one workgroup computes: one (batch, head) of attention, one
    row (LayerNorm rows; dgamma / dbeta per column), one 256 x 256 tile of gemm_tn, one image of logits -- and a failure
    reports how many units are off and the first few indices;
  * the inputs change between calls (A, then B, then A again, into the same buffers), every run is compared with its own
    reference, and every output buffer the caller owns is filled with NaN first (outputs the API ACCUMULATES into --
    LayerNorm's dx / dgamma / dbeta, gemm_tn's OUT / dbias -- start from a fresh random base per call instead);
  * every checker proves it can fail: one unit of a correct output is replaced by the output of the PREVIOUS input (the
    stale-read case) on the host, and the checker must flag exactly that unit;
  * op references are torch float64 on the GPU on the same bf16-rounded inputs; model references are the fp32 oracle on
    the GPU (checked against the CPU oracle, which tests/golden pins, in test_oracle_on_the_gpu_equals_the_oracle_on_the_cpu).
"""
import ctypes as C
import gc
import types

import numpy as np
import pytest
import torch

from kzv import _lib as L
from kzv import params as P
from kzv.config import vit_b_config
from kzv.data import build_decoder_dir, synthetic_batch
from kzv.model import TrOCRModel
from kzv.optim import RAdamScheduleFree
from oracle import trocr_oracle as O

from _replay import step_masks

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAN = float("nan")
LOGIT_TOL = 3e-2          # tests/test_model_gpu.py: bf16 GEMM operands, fp32 accumulate


@pytest.fixture(scope="module")
def lib():
    return L.load()


def _st():
    return torch.cuda.current_stream().cuda_stream


# ------------------------------------------------------------------------------------------------ unit checker
def _unit_err(got, want, ndim):
    """max |got - want| over each unit; the unit index is the first ``ndim`` dims.  NaN (an unwritten output) counts as inf."""
    d = torch.nan_to_num((got.double() - want.double()).abs(), nan=float("inf"))
    return d.reshape(*d.shape[:ndim], -1).amax(-1)


def _bad(err, tol):
    """Boolean mask of the units outside their bound (NaN-safe)."""
    return ~(err <= tol)


def _check(name, err, tol):
    """Assert every unit is within its bound; returns the worst err / tol ratio."""
    bad = _bad(err, tol)
    if bool(bad.any()):
        first = bad.nonzero()[:6].tolist()
        raise AssertionError(f"{name}: {int(bad.sum())} of {bad.numel()} units outside the bound, first {first}, "
                             f"worst error {float(err.max()):.4g}")
    return float((err / tol).max())


def _check_all(tag, results):
    """results: name -> (err, tol) per unit.  Prints the worst error and ratio of each output."""
    ratios = {k: _check(f"{tag} {k}", e, t) for k, (e, t) in results.items()}
    print(f"{tag}: " + ", ".join(f"{k} worst {float(results[k][0].max()):.3g} ({r:.2f} of bound)" for k, r in ratios.items()))
    return ratios


def _assert_flags(results, name, unit):
    """The planted-error self-check: output ``name`` must flag ``unit`` (a tuple index) and nothing else."""
    err, tol = results[name]
    bad = _bad(err, tol)
    assert bool(bad[unit]), f"the checker missed a stale {name} unit at {unit}"
    assert int(bad.sum()) == 1, f"{name}: the planted error at {unit} flagged {int(bad.sum())} units"


# ------------------------------------------------------------------------------------------------ 1. attention
# (kind, Sq): the encoder's exact 11-tile instance; decoder self-attention at the trimmed (60) and full (127) length,
# causal over the bench labels (ld_ids = 128); cross-attention over 160 patches with K / V in the 3,072-wide K/V buffer.
ATTN_CASES = [("enc", 161), ("dec_self", 60), ("dec_self", 127), ("dec_cross", 60), ("dec_cross", 127)]


def _attn_operands(kind, Sq, gen, lab):
    """Operands laid out as model.cpp lays them out (its lines for attn(): encoder 505 / 781, decoder self 551 / 728,
    cross 567 / 714).  Returns (views dict, buffers to NaN-fill, geometry)."""
    B, Hd, He = 256, 256, 768
    rnd = lambda *s: torch.randn(*s, device=DEV, generator=gen).bfloat16()
    if kind == "enc" or kind == "dec_self":
        H, heads = (He, 12) if kind == "enc" else (Hd, 4)
        qkv = rnd(B * Sq, 3 * H)
        dqkv = torch.empty_like(qkv)
        v = dict(Q=qkv[:, :H], K=qkv[:, H:2 * H], V=qkv[:, 2 * H:], dQ=dqkv[:, :H], dK=dqkv[:, H:2 * H], dV=dqkv[:, 2 * H:],
                 ldq=3 * H, ldkv=3 * H)
        Sk, mode, owned = Sq, (0 if kind == "enc" else 1), [dqkv]
    else:
        H, heads, Sk, mode, CK, layer = Hd, 4, 160, 0, 2 * Hd * 6, 5       # the last layer's K | V columns of crosskv
        cq = rnd(B * Sq, H)
        ckv = rnd(B * Sk, CK)
        dq, dckv = torch.empty_like(cq), torch.empty_like(ckv)
        c0 = layer * 2 * H
        v = dict(Q=cq, K=ckv[:, c0:c0 + H], V=ckv[:, c0 + H:c0 + 2 * H], dQ=dq, dK=dckv[:, c0:c0 + H], dV=dckv[:, c0 + H:c0 + 2 * H],
                 ldq=H, ldkv=CK, dckv=dckv, c0=c0)
        owned = [dq, dckv]
    v["O"] = torch.empty(B * Sq, H, dtype=torch.bfloat16, device=DEV)
    v["dO"] = rnd(B * Sq, H)
    v["LSE"] = torch.empty(B, heads, Sq, device=DEV)
    v["ids"] = lab if mode == 1 else None
    owned += [v["O"], v["LSE"]]
    return v, owned, types.SimpleNamespace(B=B, H=H, heads=heads, Sq=Sq, Sk=Sk, mode=mode)


def _attn_run(lib, v, owned, g, drop, key):
    for t in owned:
        t.fill_(NAN)
    a = L.kzv_attn_args(Q=v["Q"].data_ptr(), K=v["K"].data_ptr(), V=v["V"].data_ptr(), O=v["O"].data_ptr(), LSE=v["LSE"].data_ptr(),
                        dO=v["dO"].data_ptr(), dQ=v["dQ"].data_ptr(), dK=v["dK"].data_ptr(), dV=v["dV"].data_ptr(),
                        ldq=v["ldq"], ldk=v["ldkv"], ldv=v["ldkv"], ldo=g.H, ids=L.ptr(v["ids"]), ld_ids=128, pad_id=1,
                        B=g.B, heads=g.heads, Sq=g.Sq, Sk=g.Sk, mode=g.mode, drop_p=drop, drop_key=key)
    L.check(lib.kzv_attn_fwd(C.byref(a), _st()), "attn_fwd")
    L.check(lib.kzv_attn_bwd(C.byref(a), _st()), "attn_bwd")
    torch.cuda.synchronize()
    heads_view = lambda t, S: t.view(g.B, S, g.heads, 64).transpose(1, 2)          # [B, heads, S, 64]: unit = (b, h)
    out = {"O": heads_view(v["O"], g.Sq), "LSE": v["LSE"], "dQ": heads_view(v["dQ"], g.Sq), "dK": heads_view(v["dK"], g.Sk),
           "dV": heads_view(v["dV"], g.Sk)}
    out = {k: t.clone() for k, t in out.items()}
    if "dckv" in v:        # nothing outside this layer's K | V columns may be written
        rest = torch.cat([v["dckv"][:, :v["c0"]], v["dckv"][:, v["c0"] + 2 * g.H:]], 1)
        assert bool(rest.isnan().all()), "attn_bwd wrote outside the dK / dV columns"
    return out


def _attn_ref(lib, v, g, drop, key):
    """float64 forward / backward of softmax(q k^T / 8 [+ causal & key-not-pad mask]) [x dropout multipliers] v on the
    bf16 operands; the dropout multipliers are the ones kzv_debug_attn_dropout_mask reports for (key, p)."""
    qh, kh, vh = (t.double().view(g.B, -1, g.heads, 64).transpose(1, 2).requires_grad_(True) for t in (v["Q"], v["K"], v["V"]))
    s = qh @ kh.transpose(2, 3) * 0.125
    if g.mode == 1:
        ids = v["ids"][:, :g.Sk]
        keep = torch.ones(g.Sq, g.Sk, dtype=torch.bool, device=DEV).tril()[None, None] & (ids != 1)[:, None, None, :]
        s = s.masked_fill(~keep, float("-inf"))
    p = torch.softmax(s, -1)
    if drop > 0:
        m = torch.empty(g.B * g.heads * g.Sq, g.Sk, device=DEV)
        L.check(lib.kzv_debug_attn_dropout_mask(key, drop, g.B * g.heads, g.Sq, g.Sk, m.data_ptr(), _st()), "mask")
        p = p * m.view(g.B, g.heads, g.Sq, g.Sk).double()
    o = p @ vh
    dq, dk, dv = torch.autograd.grad(o, (qh, kh, vh), v["dO"].double().view(g.B, g.Sq, g.heads, 64).transpose(1, 2))
    return {"O": o.detach(), "LSE": torch.logsumexp(s.detach(), -1), "dQ": dq, "dK": dk, "dV": dv}


def _attn_compare(got, ref):
    """Per (batch, head).  Bounds of tests/test_ops_gpu.py::test_attention_fwd_bwd, per unit: P and the outputs are rounded to
    bf16 (2^-8 relative) around 64..161-term sums -> O within 0.02, dQ / dK / dV within 0.03 of max(1, the unit's largest
    entry); LSE (fp32 throughout) within 2e-3."""
    res = {}
    for k, want in ref.items():
        err = _unit_err(got[k], want, 2)
        if k == "LSE":
            tol = torch.full_like(err, 2e-3)
        else:
            tol = (0.02 if k == "O" else 0.03) * want.abs().reshape(*want.shape[:2], -1).amax(-1).clamp(min=1.0)
        res[k] = (err, tol)
    return res


@pytest.mark.parametrize("drop", [0.0, 0.1])
@pytest.mark.parametrize("kind,Sq", ATTN_CASES)
def test_attention_at_the_model_strides(lib, bench, kind, Sq, drop):
    """kzv_attn_fwd / kzv_attn_bwd at B = 256 (3,072 encoder workgroups, 1,024 decoder ones) with the model's packed layouts,
    dropout off and 0.1 (explicit masks from kzv_debug_attn_dropout_mask, another key per input); causal cases over the labels
    of the bench batch and of the second batch.  O, LSE, dQ, dK, dV per (batch, head) against float64; bounds in
    _attn_compare; observed on MI355X: at most 0.24 (O), 0.36 (dQ / dK / dV) and 0.001 (LSE) of the bound.  Inputs A, B, A
    into the same NaN-filled buffers."""
    gen = torch.Generator(device=DEV)
    labs = {1: torch.from_numpy(bench.inputs["A"][1]).to(DEV), 2: torch.from_numpy(bench.inputs["B"][1]).to(DEV)}
    gen.manual_seed(1000 + Sq)
    va, owned, g = _attn_operands(kind, Sq, gen, labs[1])
    gen.manual_seed(2000 + Sq)
    vb, _, _ = _attn_operands(kind, Sq, gen, labs[2])
    # B's operands go through A's buffers: copy them in before B's run, back after
    keys = {"A": 77 + Sq, "B": 91 + Sq}
    refs = {"A": _attn_ref(lib, va, g, drop, keys["A"]), "B": _attn_ref(lib, vb, g, drop, keys["B"])}
    saved = {k: va[k].clone() for k in ("Q", "K", "V", "dO")}
    saved["ids"] = va["ids"]
    runs = []
    for which in ("A", "B", "A"):
        src = vb if which == "B" else saved
        for k in ("Q", "K", "V", "dO"):
            va[k].copy_(src[k])
        va["ids"] = src["ids"]
        got = _attn_run(lib, va, owned, g, drop, keys[which])
        _check_all(f"{kind} Sq={Sq} p={drop} input {which}", _attn_compare(got, refs[which]))
        runs.append(got)
    # self-check: one 16-row tile of one head (one head's LSE rows) of the last A run replaced by the B run's; causal: an
    # image with >= 40 characters in both batches (padded keys have dK = dV = 0 in both)
    b, h, r = g.B - 3, g.heads - 1, 16
    if g.mode == 1:
        b = int((((labs[1] != 1).sum(1) >= 40) & ((labs[2] != 1).sum(1) >= 40)).nonzero()[0])
    for name in ("O", "LSE", "dQ", "dK", "dV"):
        planted = {k: t.clone() for k, t in runs[2].items()}
        planted[name][b, h, r:r + 16] = runs[1][name][b, h, r:r + 16]
        _assert_flags(_attn_compare(planted, refs["A"]), name, (b, h))


# ------------------------------------------------------------------------------------------------ 2. LayerNorm
LN_EPS = 1e-12


def _ln_inputs(rows, H, seed):
    gen = torch.Generator(device=DEV).manual_seed(seed)
    x = torch.randn(rows, H, device=DEV, generator=gen) * 2 + 0.5
    g = 1 + 0.1 * torch.randn(H, device=DEV, generator=gen)
    b = 0.1 * torch.randn(H, device=DEV, generator=gen)
    dy = torch.randn(rows, H, device=DEV, generator=gen)
    return x, g, b, dy


def _ln_ref(x, g, b, dy):
    """float64 LayerNorm forward, statistics, and the gradients of <y, dy> for the given (fp32 or bf16-rounded) dy;
    also the per-column sums of |dy * xhat| and |dy| the dgamma / dbeta bounds scale with."""
    xd, gd, bd = (t.double().requires_grad_(True) for t in (x, g, b))
    y = torch.nn.functional.layer_norm(xd, (x.shape[1],), gd, bd, LN_EPS)
    mean = xd.detach().mean(1)
    var = xd.detach().var(1, unbiased=False)
    rstd = (var + LN_EPS).rsqrt()
    out = {"y": y.detach(), "mean": mean, "rstd": rstd}
    xhat = (xd.detach() - mean[:, None]) * rstd[:, None]
    for tag, d in (("32", dy), ("16", dy.bfloat16())):
        dx, dg, db = torch.autograd.grad(y, (xd, gd, bd), d.double(), retain_graph=True)
        out["dx" + tag], out["dg" + tag], out["db" + tag] = dx, dg, db
        out["sg" + tag] = (d.double() * xhat).abs().sum(0)
        out["sb" + tag] = d.double().abs().sum(0)
    return out


def _ln_compare(got, ref, tag):
    """Forward per row: y (fp32) within 2e-5 (test_layernorm_fwd_bwd's bound), y (bf16) within 2^-8 of the row's largest
    |y|, mean within 1e-5 of the row's largest |x|, rstd within 1e-5 relative (fp32 sums of H terms: ~1e-6 observed in
    kind).  Backward: dx per row within 3e-5 of max(1, the row's largest |dx|) (fp32 dy: test_layernorm_fwd_bwd's bound; the
    bf16 dy is rounded in the reference too, so the same); dgamma / dbeta per column within 4e-6 of the column's sum of |terms|
    -- a few fp32 roundings of partial sums; one 64-row workgroup's share missing from a column is ~1e-3 of that sum."""
    res = {}
    if "y32" in got:
        res["y32"] = (_unit_err(got["y32"], ref["y"], 1), torch.full((ref["y"].shape[0],), 2e-5, device=DEV, dtype=torch.float64))
        res["y16"] = (_unit_err(got["y16"], ref["y"], 1), (2 ** -8 + 1e-6) * ref["y"].abs().amax(1))
        res["mean"] = (_unit_err(got["mean"], ref["mean"], 1), 1e-5 * ref["xmax"])
        res["rstd"] = (_unit_err(got["rstd"], ref["rstd"], 1), 1e-5 * ref["rstd"])
    if "dx" in got:
        res["dx"] = (_unit_err(got["dx"], ref["dx" + tag], 1), 3e-5 * ref["dx" + tag].abs().amax(1).clamp(min=1.0))
        res["dgamma"] = (_unit_err(got["dg"], ref["dg" + tag], 1), 4e-6 * ref["sg" + tag])
        res["dbeta"] = (_unit_err(got["db"], ref["db" + tag], 1), 4e-6 * ref["sb" + tag])
    return res


@pytest.mark.parametrize("rows,H", [(41216, 768), (32512, 256), (15360, 256)])
def test_layernorm_at_the_bench_row_counts(lib, rows, H):
    """kzv_layernorm_fwd / kzv_layernorm_bwd (accumulate_dx on; dy fp32 and bf16) at the encoder's 41,216 x 768 (10,304 forward
    workgroups) and the decoder's untrimmed 32,512 and trimmed 15,360 x 256 rows; dgamma / dbeta are float-atomic sums from
    64-row workgroups into 32 slots.  y, stats and dx per row, dgamma / dbeta per column against float64 (bounds in
    _ln_compare; observed on MI355X: y32 0.05, y16 0.99 (one bf16 rounding: the bound is that rounding's), mean 0.00, rstd 0.01,
    dx 0.01, dgamma / dbeta 0.00 of the bound).  Inputs A, B, A; outputs NaN-filled, accumulated ones on a fresh random base."""
    inputs = {"A": _ln_inputs(rows, H, rows + H), "B": _ln_inputs(rows, H, rows + H + 1)}
    refs = {k: _ln_ref(*v) for k, v in inputs.items()}
    for k, (x, _, _, _) in inputs.items():
        refs[k]["xmax"] = x.double().abs().amax(1)
    x, g, b, dy = (t.clone() for t in inputs["A"])
    y16 = torch.empty(rows, H, dtype=torch.bfloat16, device=DEV)
    y32 = torch.empty(rows, H, device=DEV)
    stats = torch.empty(rows, 2, device=DEV)
    dx, dg, db = torch.empty(rows, H, device=DEV), torch.empty(H, device=DEV), torch.empty(H, device=DEV)
    base_gen = torch.Generator(device=DEV).manual_seed(5)
    runs = []
    for which in ("A", "B", "A"):
        for dst, src in zip((x, g, b, dy), inputs[which]):
            dst.copy_(src)
        for t in (y16, y32, stats):
            t.fill_(NAN)
        L.check(lib.kzv_layernorm_fwd(x.data_ptr(), g.data_ptr(), b.data_ptr(), y16.data_ptr(), y32.data_ptr(), stats.data_ptr(),
                                      rows, H, LN_EPS, _st()), "ln_fwd")
        got = {"y32": y32.clone(), "y16": y16.clone(), "mean": stats[:, 0].clone(), "rstd": stats[:, 1].clone()}
        _check_all(f"ln {rows}x{H} fwd input {which}", _ln_compare(got, refs[which], "32"))
        fwd = got
        for is32, tag in ((1, "32"), (0, "16")):
            dy_in = dy if is32 else dy.bfloat16()
            bases = [torch.randn(t.shape, device=DEV, generator=base_gen) for t in (dx, dg, db)]
            for t, base in zip((dx, dg, db), bases):
                t.copy_(base)
            L.check(lib.kzv_layernorm_bwd(dy_in.data_ptr(), is32, x.data_ptr(), stats.data_ptr(), g.data_ptr(), dx.data_ptr(), 1,
                                          dg.data_ptr(), db.data_ptr(), rows, H, _st()), "ln_bwd")
            got = {"dx": dx - bases[0], "dg": dg - bases[1], "db": db - bases[2]}
            _check_all(f"ln {rows}x{H} bwd dy{tag} input {which}", _ln_compare(got, refs[which], tag))
            if tag == "32":
                fwd.update(got)
        runs.append(fwd)
    # self-check: one 64-row block (one column of dgamma / dbeta) of the last A run replaced by the B run's
    r, c = 64 * (rows // 64 // 3), H // 2 + 3
    for name, unit in (("y32", "y32"), ("y16", "y16"), ("mean", "mean"), ("rstd", "rstd"), ("dx", "dx"), ("dg", "dgamma"), ("db", "dbeta")):
        planted = {k: t.clone() for k, t in runs[2].items()}
        if name in ("dg", "db"):
            planted[name][c] = runs[1][name][c]
            _assert_flags(_ln_compare(planted, refs["A"], "32"), unit, (c,))
        else:
            planted[name][r:r + 64] = runs[1][name][r:r + 64]
            err, tol = _ln_compare(planted, refs["A"], "32")[unit]
            bad = _bad(err, tol)
            assert bool(bad[r:r + 64].all()) and int(bad.sum()) == 64, (unit, int(bad.sum()))


# ------------------------------------------------------------------------------------------------ 3. gemm_tn
def _tn_compare(out, db, ref, dbref, Mt):
    """Per 256 x 256 tile of OUT: test_gemm_tn_large_outputs_take_the_256x256_kernel's bound (the token splits' partial tiles
    cross the workspace as bf16) applied to the tile's own largest entry: 4e-3 x max |tile| + 2e-3; dbias per column
    within 2e-3 sqrt(Mtok / 4096) + 2e-3 (the same test's bound)."""
    N, K = ref.shape
    tiles = lambda t: t.reshape(N // 256, 256, K // 256, 256).transpose(1, 2)
    e = _unit_err(tiles(out), tiles(ref), 2)
    tol = 4e-3 * tiles(ref).abs().reshape(N // 256, K // 256, -1).amax(-1) + 2e-3
    return {"OUT": (e, tol), "dbias": (_unit_err(db, dbref, 1), torch.full((N,), 2e-3 * (Mt / 4096) ** 0.5 + 2e-3, device=DEV))}


@pytest.mark.parametrize("reserve", [0, 32])
@pytest.mark.parametrize("Mt,N,K", [(41216, 2304, 768), (41216, 768, 768), (41216, 3072, 768), (41216, 768, 3072), (32512, 768, 256)])
def test_gemm_tn_weight_gradients_at_the_bench_token_count(lib, Mt, N, K, reserve):
    """kzv_gemm_tn (OUT += P^T Q, dbias += column sums of P) on the encoder's four weight-gradient shapes at 41,216 tokens (644
    token tiles in 7..28 splits) and the decoder's untrimmed 32,512 tokens at (768, 256); the default plan and
    kzv_set_cu_reserve(32), which changes the split count (the setting found is restored).  Per-tile bounds in _tn_compare;
    observed on MI355X: at most 0.69 of the bound per tile at 41,216 tokens (0.00 at 32,512: one split), dbias 0.03.  Inputs
    A, B, A, each call on a fresh random OUT / dbias base."""
    gen = torch.Generator(device=DEV).manual_seed(Mt + N + K)
    inputs = {w: (torch.randn(Mt, N, device=DEV, generator=gen).bfloat16(), torch.randn(Mt, K, device=DEV, generator=gen).bfloat16())
              for w in ("A", "B")}
    refs = {w: (Pm.double().t() @ Q.double(), Pm.double().sum(0)) for w, (Pm, Q) in inputs.items()}
    Pm, Q = (t.clone() for t in inputs["A"])
    out, db = torch.empty(N, K, device=DEV), torch.empty(N, device=DEV)
    a = L.kzv_gemm_tn_args(P=Pm.data_ptr(), ldp=N, Q=Q.data_ptr(), ldq=K, OUT=out.data_ptr(), ldo=K, Mtok=Mt, N=N, K=K, n_store=N,
                           dbias=db.data_ptr())
    runs = []
    found = lib.kzv_get_cu_reserve()
    try:
        L.check(lib.kzv_set_cu_reserve(reserve), "set_cu_reserve")
        for which in ("A", "B", "A"):
            Pm.copy_(inputs[which][0]); Q.copy_(inputs[which][1])
            base, dbase = torch.randn(N, K, device=DEV, generator=gen), torch.randn(N, device=DEV, generator=gen)
            out.copy_(base); db.copy_(dbase)
            L.check(lib.kzv_gemm_tn(C.byref(a), _st()), "gemm_tn")
            torch.cuda.synchronize()
            got = (out.double() - base, db.double() - dbase)
            _check_all(f"gemm_tn {Mt}x({N},{K}) reserve {reserve} input {which}", _tn_compare(*got, *refs[which], Mt))
            runs.append(got)
    finally:
        L.check(lib.kzv_set_cu_reserve(found), "set_cu_reserve")
    # self-check: one 256 x 256 tile (one dbias column) of the last A run replaced by the B run's
    tn, tk, c = N // 256 - 1, K // 256 // 2, N // 3
    planted = runs[2][0].clone()
    planted[tn * 256:(tn + 1) * 256, tk * 256:(tk + 1) * 256] = runs[1][0][tn * 256:(tn + 1) * 256, tk * 256:(tk + 1) * 256]
    _assert_flags(_tn_compare(planted, runs[2][1], *refs["A"], Mt), "OUT", (tn, tk))
    planted = runs[2][1].clone()
    planted[c] = runs[1][1][c]
    _assert_flags(_tn_compare(runs[2][0], planted, *refs["A"], Mt), "dbias", (c,))


# ------------------------------------------------------------------------------------------------ 5. optimizer
def test_clip_and_radam_schedulefree_on_the_bench_model_size():
    """RAdamScheduleFree.step (the grad-norm + clip_step kernels) over a flat buffer the size of the bench model's,
    92,705,792 floats, 7 steps with ||g|| ~ 3 (clip 1.0 active): steps 1-5 are the silent phase, 6-7 adaptive.  Reference:
    the oracle's radam_schedulefree_step in float64 (run on the GPU's float64 tensors).  Per element, the bounds of
    test_clip_and_radam_schedulefree_kernels_match_oracle: 1e-5 relative + 1e-8 (v: 1e-14); the norm within 1e-5.  Observed on
    MI355X: at most 0.022 (p), 0.017 (z), 0.010 (v) of the bound."""
    n = P.param_offsets(vit_b_config(dec_layers=6))[1]
    assert n == 92_705_792
    gen = torch.Generator(device=DEV).manual_seed(11)
    p0 = torch.randn(n, device=DEV, generator=gen) * 0.02

    fm = types.SimpleNamespace(flat_params=p0.clone(), flat_grads=torch.zeros_like(p0), sync_weights=lambda: None)
    opt = RAdamScheduleFree(fm, lr=1e-3, betas=(0.9, 0.999), eps=1e-8)
    st = O.RAdamScheduleFreeState(lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8)
    y = p0.double(); z = y.clone(); v = torch.zeros_like(y)
    phases, prev = set(), None

    def compare(got, want):
        res = {}
        for name in ("p", "z", "v"):
            err = torch.nan_to_num((got[name].double() - want[name]).abs(), nan=float("inf"))
            res[name] = (err, 1e-5 * want[name].abs() + (1e-8 if name != "v" else 1e-14))
        return res

    for step in range(7):
        g = torch.randn(n, device=DEV, generator=gen) * 3e-4 * (1 + step % 3)
        fm.flat_grads.copy_(g)
        opt.step(max_grad_norm=1.0)
        phases.add(opt.scheduled_lr > 0)
        total = float(g.double().norm())                  # O.clip_grad_norm, on the device
        coef = min(1.0, 1.0 / (total + 1e-6))
        assert coef < 0.5 and abs(opt.grad_norm() - total) <= 1e-5 * total, (step, opt.grad_norm(), total)
        O.radam_schedulefree_step(st, y, z, v, g.double() * coef)
        got = {"p": fm.flat_params.clone(), "z": opt.z.clone(), "v": opt.v.clone()}
        res = compare(got, {"p": y, "z": z, "v": v})
        worst = {k: float((e / t).max()) for k, (e, t) in res.items()}
        for k, (e, t) in res.items():
            _check(f"optimizer step {step + 1} {k}", e, t)
        print(f"optimizer step {step + 1}: worst err / bound " + ", ".join(f"{k} {r:.3g}" for k, r in worst.items()))
        if step < 6:
            prev = got
    assert phases == {True, False}
    # self-check: one 256-element block of the last step's p replaced by the step before's (the adaptive phase moves p)
    i = n // 2 + 256 * 7
    got["p"][i:i + 256] = prev["p"][i:i + 256]
    err, tol = compare(got, {"p": y, "z": z, "v": v})["p"]
    bad = _bad(err, tol)
    assert bool(bad[i:i + 256].any()) and not bool(bad[:i].any()) and not bool(bad[i + 256:].any())


# ------------------------------------------------------------------------------------------------ 4. the whole model
SEED = 4242
ORACLE_CHUNKS = 4         # images per oracle call: 64 (keeps the fp32 oracle's saved activations near 10 GB)


def _no_dropout(cfg):
    import dataclasses
    return dataclasses.replace(cfg, enc_hidden_dropout=0.0, enc_attn_dropout=0.0, dec_hidden_dropout=0.0, dec_attn_dropout=0.0)


def _oracle(cfg, sd, px, lab, masks=None):
    """oracle.forward_backward on the GPU over ORACLE_CHUNKS slices of the images (each image's dropout masks go with it):
    the loss is the token-count-weighted mean of the slices' losses and each gradient the same weighted sum (in float64) --
    the mean-over-tokens loss of the whole batch, exactly."""
    n = px.shape[0] // ORACLE_CHUNKS
    tgt = lab[:, 1:] != cfg.pad_id
    out = {"logits": [], "loss": 0.0, "grads": {}}
    for c in range(ORACLE_CHUNKS):
        sl = slice(c * n, (c + 1) * n)
        w = float(tgt[sl].sum()) / float(tgt.sum())
        r = O.forward_backward(cfg, sd, px[sl], lab[sl], masks=None if masks is None else {k: v[sl] for k, v in masks.items()},
                               device=DEV)
        out["logits"].append(r["logits"])
        out["loss"] += w * r["loss"]
        for k, g in r["grads"].items():
            if g is not None:
                out["grads"][k] = out["grads"].get(k, 0.0) + w * g.astype(np.float64)
            else:
                out["grads"].setdefault(k, None)
    out["logits"] = np.concatenate(out["logits"])
    torch.cuda.empty_cache()
    return out


@pytest.fixture(scope="module")
def bench():
    """The benchmark's configuration, weights and batch (A), and a second batch of the same shape (B).  ``ref(which)``: the
    fp32 oracle on the GPU, dropout off, cached."""
    cfg = vit_b_config(dec_layers=6)
    ns = types.SimpleNamespace(cfg=cfg, sd=P.state_dict_from_flat(cfg, P.recipe_flat(cfg, 42)), refs={})
    ns.inputs = {"A": synthetic_batch(cfg, 256, 128, seed=1), "B": synthetic_batch(cfg, 256, 128, seed=2)}

    def ref(which):
        if which not in ns.refs:
            ns.refs[which] = _oracle(cfg, ns.sd, *ns.inputs[which])
        return ns.refs[which]
    ns.ref = ref
    return ns


def _engine(cfg, tmp_path):
    """A bench engine (init_seed 42) of its own per test, so that one B = 256 workspace is allocated at a time."""
    m = TrOCRModel(cfg.encoder_config_dict(), build_decoder_dir(str(tmp_path / "dec"), cfg), init_seed=42, load_tokenizer=False)
    yield m
    del m
    gc.collect()
    torch.cuda.empty_cache()


@pytest.fixture
def drop_engine(bench, tmp_path):
    yield from _engine(bench.cfg, tmp_path)


@pytest.fixture
def nodrop_engine(bench, tmp_path):
    yield from _engine(_no_dropout(bench.cfg), tmp_path)


def _grad_errors(cfg, got_flat, ref_grads):
    """Per gradient tensor: max |got - want| / max |want| (the key biases' true gradient is exactly 0 -- softmax is invariant
    to a per-query shift -- and the tied LM-head alias is the word embedding: both skipped, as in test_model_gpu.py)."""
    got = P.state_dict_from_flat(cfg, got_flat)
    out = {}
    for k, want in ref_grads.items():
        if want is None or k.endswith("key.bias") or k.startswith("decoder.lm_head.decoder."):
            continue
        w = want if torch.is_tensor(want) else torch.from_numpy(np.asarray(want)).to(DEV)
        w = w.reshape(-1).double()
        d = torch.nan_to_num((got[k].reshape(-1).double() - w).abs(), nan=float("inf"))
        out[k] = float(d.max()) / (float(w.abs().max()) + 1e-12)
    return out


def _check_grads(tag, worst, max_tol, median_tol):
    bad = {k: e for k, e in worst.items() if not e <= max_tol}
    med = float(np.median(list(worst.values())))
    print(f"{tag}: {len(worst)} gradient tensors, worst relative error {max(worst.values()):.4g} "
          f"({max(worst, key=worst.get)}), median {med:.4g}")
    assert not bad, (tag, len(bad), sorted(bad.items(), key=lambda kv: -kv[1])[:6])
    assert med <= median_tol, (tag, med)


def test_oracle_on_the_gpu_equals_the_oracle_on_the_cpu():
    """The model-level reference itself: oracle.forward_backward on the GPU against the CPU oracle (the one tests/golden pins)
    at ViT-B, B = 2, with the dropout masks of a real step replayed on both devices: logits within 1e-4 of max(1, max |logit|),
    loss within 1e-4, every gradient tensor within 1e-4 of its largest entry (fp32 on both; the summation orders differ)."""
    cfg = vit_b_config(dec_layers=6)
    sd = P.state_dict_from_flat(cfg, P.recipe_flat(cfg, 42))
    px, lab = synthetic_batch(cfg, 2, 40, seed=3, min_chars=3, max_chars=39)
    masks = step_masks(cfg, 99, 2, 39, device=DEV)
    cpu = O.forward_backward(cfg, sd, px, lab, masks={k: v.cpu() for k, v in masks.items()})
    gpu = O.forward_backward(cfg, sd, px, lab, masks=masks, device=DEV)
    err = float(np.abs(gpu["logits"] - cpu["logits"]).max())
    print(f"oracle gpu vs cpu: max|dlogit| {err:.3g}, |dloss| {abs(gpu['loss'] - cpu['loss']):.3g}")
    assert err <= 1e-4 * max(1.0, float(np.abs(cpu["logits"]).max()))
    assert abs(gpu["loss"] - cpu["loss"]) <= 1e-4
    worst = {}
    for k, want in cpu["grads"].items():
        if want is None or k.endswith("key.bias"):
            continue
        worst[k] = float(np.abs(gpu["grads"][k] - want).max() / (np.abs(want).max() + 1e-12))
    print(f"oracle gpu vs cpu: worst relative gradient difference {max(worst.values()):.3g}")
    assert max(worst.values()) <= 1e-4, sorted(worst.items(), key=lambda kv: -kv[1])[:5]


def _logit_compare(got, want):
    """Per image: max |logit - oracle| within LOGIT_TOL."""
    return {"logits": (_unit_err(got, want, 1), torch.full((got.shape[0],), LOGIT_TOL, device=DEV, dtype=torch.float64))}


def test_logits_of_all_256_images_against_the_gpu_oracle(bench, drop_engine):
    """Eval mode, the bench model and batch (and a second batch B; order A, B, A): the logits of every position of all 256
    images (want_logits computes the full 127 positions: the untrimmed decoder, 508 chain workgroups) per image within
    LOGIT_TOL of the fp32 oracle (test_model_gpu.py's bound); the loss within 5e-3; argmax equal wherever the oracle's top-2
    gap exceeds twice that image's error (observed: ~90 % of the positions)."""
    m = drop_engine
    m.eval()
    runs = []
    for which in ("A", "B", "A"):
        px, lab = bench.inputs[which]
        r = bench.ref(which)
        loss, logits = m.forward_loss(torch.from_numpy(px), torch.from_numpy(lab), want_logits=True, seed=SEED)
        torch.cuda.synchronize()
        want = torch.from_numpy(r["logits"]).to(DEV)
        res = _logit_compare(logits, want)
        _check_all(f"logits input {which}", res)
        assert abs(float(loss.item()) - r["loss"]) < 5e-3
        top2 = want.topk(2, -1).values
        decided = (top2[..., 0] - top2[..., 1]) > 2 * res["logits"][0][:, None]
        agree = logits.argmax(-1) == want.argmax(-1)
        print(f"logits input {which}: |dloss| {abs(float(loss.item()) - r['loss']):.3g}, decided positions "
              f"{float(decided.float().mean()):.3f}, argmax agreement {float(agree.float().mean()):.4f}")
        assert bool(agree[decided].all()), int((~agree & decided).sum())
        assert float(decided.float().mean()) > 0.8
        runs.append(logits.clone())
    # self-check: one image of the last A run replaced by the B run's
    planted = runs[2].clone()
    planted[137] = runs[1][137]
    _assert_flags(_logit_compare(planted, torch.from_numpy(bench.ref("A")["logits"]).to(DEV)), "logits", (137,))


@pytest.mark.parametrize("trim", [True, False])
def test_gradients_of_the_bench_batch_against_the_gpu_oracle(bench, nodrop_engine, trim):
    """Dropout off, trim_padding on (the headline's decoder geometry: 60 positions -- trimmed steps return no logits, so this
    is the only reference check of it) and off (127): loss within 5e-3 and every gradient tensor of the 256-image batch
    against the fp32 oracle with test_model_gpu.py's per-tensor bounds (max <= 0.05 of the tensor's largest entry,
    median <= 0.02; observed 0.038 / 0.008).  Inputs A, B, A; flat_grads NaN-filled before every step."""
    m, cfg = nodrop_engine, bench.cfg
    m.train()
    m.trim_padding = trim
    got = {}
    for which in ("A", "B", "A"):
        px, lab = bench.inputs[which]
        r = bench.ref(which)
        m.flat_grads.fill_(NAN)
        loss, _ = m.forward_loss(torch.from_numpy(px), torch.from_numpy(lab), seed=SEED)
        m.backward()
        torch.cuda.synchronize()
        assert m.last_active_length == (60 if trim else 127)
        dl = abs(float(loss.item()) - r["loss"])
        worst = _grad_errors(cfg, m.flat_grads, r["grads"])
        print(f"grads trim={trim} input {which}: |dloss| {dl:.3g}")
        assert dl < 5e-3
        _check_grads(f"grads trim={trim} input {which}", worst, 0.05, 0.02)
        got[which] = m.flat_grads.clone()
    # self-check: one gradient tensor of the last A step replaced by the B step's
    name = "encoder.encoder.layer.0.attention.attention.query.weight"
    planted = got["A"].clone()
    P.state_dict_from_flat(cfg, planted)[name].copy_(P.state_dict_from_flat(cfg, got["B"])[name])
    worst = _grad_errors(cfg, planted, bench.ref("A")["grads"])
    assert worst[name] > 0.05 and sum(e > 0.05 for e in worst.values()) == 1, worst[name]


def test_the_bench_step_with_dropout_replayed_through_the_gpu_oracle(bench, drop_engine):
    """One dropout-on step of the bench model on the bench batch (trimmed to 60 positions, as timed) at an explicit seed; its
    masks (step_masks(cfg, seed, 256, 60) on the device) replayed through the fp32 oracle on the GPU, as
    test_parity_gpu.py::_replay_case does: loss within 5e-3, every gradient tensor within 0.06 of its largest entry (that
    test's ViT-B bound), median within 0.02 (observed 0.025 / 0.009); and the masks matter: the dropout-off gradients miss
    that bound for most tensors.  Prints the peak of torch.cuda.max_memory_allocated."""
    m, cfg = drop_engine, bench.cfg
    px, lab = bench.inputs["A"]
    nomask = bench.ref("A")["grads"]
    torch.cuda.reset_peak_memory_stats()
    m.train()
    m.flat_grads.fill_(NAN)
    loss, _ = m.forward_loss(torch.from_numpy(px), torch.from_numpy(lab), seed=SEED)
    m.backward()
    torch.cuda.synchronize()
    T = m.last_active_length
    assert T == 60
    masks = step_masks(cfg, SEED, 256, T, device=DEV)
    assert len(masks) == 1 + 3 * cfg.enc_layers + 1 + 5 * cfg.dec_layers
    r = _oracle(cfg, bench.sd, px, lab[:, :T + 1], masks=masks)       # the trimmed label columns are all padding
    del masks
    peak = torch.cuda.max_memory_allocated() / 2 ** 30
    print(f"dropout replay: |dloss| {abs(float(loss.item()) - r['loss']):.3g}; peak torch allocation {peak:.1f} GiB")
    assert abs(float(loss.item()) - r["loss"]) < 5e-3
    _check_grads("dropout replay", _grad_errors(cfg, m.flat_grads, r["grads"]), 0.06, 0.02)
    off = _grad_errors(cfg, _flat_from(cfg, nomask), r["grads"])
    missed = sum(e > 0.06 for e in off.values())
    print(f"dropout replay: without the masks {missed} of {len(off)} tensors miss the bound (median {np.median(list(off.values())):.3g})")
    assert missed > len(off) // 2


def _flat_from(cfg, grads):
    """A gradient dict (HF names) as one flat device buffer in the engine's layout."""
    flat = torch.zeros(P.param_offsets(cfg)[1], device=DEV)
    views = P.state_dict_from_flat(cfg, flat)
    for k, g in grads.items():
        if g is not None and not k.startswith("decoder.lm_head.decoder."):
            views[k].copy_(torch.from_numpy(np.asarray(g)).reshape(views[k].shape))
    return flat


def _step_grads(m, px, lab):
    """One dropout-off step of engine ``m``; returns (loss, flat gradients in float64).  flat_grads is NaN-filled first."""
    m.flat_grads.fill_(NAN)
    loss, _ = m.forward_loss(torch.from_numpy(np.ascontiguousarray(px)), torch.from_numpy(np.ascontiguousarray(lab)), seed=SEED)
    m.backward()
    torch.cuda.synchronize()
    return float(loss.item()), m.flat_grads.double()


def _rel_diff(cfg, a, b):
    """Per gradient tensor: max |a - b| / max |b| (key biases and the tied LM-head alias skipped, as in _grad_errors)."""
    return _grad_errors(cfg, a, P.state_dict_from_flat(cfg, b))


DECOMP_MAX, DECOMP_MEDIAN = 6e-3, 1e-5


def test_batch_256_equals_the_sum_of_16_batches_of_16(bench, nodrop_engine):
    """Dropout off, trim on.  Batch 256 (3,072 encoder attention workgroups, more than the CUs; 41,216 tokens in gemm_tn) against
    the same images as 16 batches of 16 (192 workgroups, fewer than the CUs; decoder chains of 32; 2,576 tokens): the loss
    equals the mean of the 16 losses and every gradient tensor the mean of the 16 gradients.
    The images are the bench batch's; every label holds 60 characters (the headline's 60 decoder positions), so each image
    has 59 targets and count = 16 x count_i exactly.  The loss gradient enters the backward as bf16 (softmax - onehot) / count:
    with a power-of-two count ratio those bf16 values, and every per-row bf16 rounding after them, are exactly 1/16 of the
    sub-batch's.  What can still differ is the order of float-atomic sums (LayerNorm dgamma / dbeta, embedding and bias
    gradients) and gemm_tn's bf16 split partials, whose splits follow the token count.  (With the bench's own labels the
    counts are not in a power-of-two ratio, every dlogit rounds differently and the two sums differ by bf16 backward noise
    as large as against the oracle: median 0.008 of the largest entry.)
    Observed on MI355X, per tensor relative to its largest entry: median 2e-7 (fp32 summation order only), 90 % 2.1e-3, worst
    3.9e-3 -- the weight gradients that gemm_tn sums over the tokens, within its per-tile bound of 4e-3 (test above); the loss
    1.4e-8 .. 5.9e-7 relative over five runs (a float-atomic sum over 15,104 tokens: its order changes from run to run).
    Bounds: every tensor within DECOMP_MAX = 6e-3 (1.5x the worst), the median within DECOMP_MEDIAN = 1e-5, the loss within
    5e-6 relative (8x the largest observed; against the oracle the loss bound is 5e-3).
    Self-check: one image's share of the batch-256 gradient (1/256 of it: 161 of 41,216 encoder tokens, 12 of 3,072
    attention workgroups) swapped for another image's share -- the stale-input case at the
    granularity of one image -- must be flagged in every tensor (observed: 3.3x DECOMP_MAX in the least sensitive tensor,
    13x at the median; a 64-token gemm_tn share is about 0.4 of an image's)."""
    m, cfg = nodrop_engine, bench.cfg
    px = bench.inputs["A"][0]
    lab = synthetic_batch(cfg, 256, 128, seed=1, min_chars=60, max_chars=60)[1]
    px_o, lab_o = synthetic_batch(cfg, 256, 128, seed=2, min_chars=60, max_chars=60)
    m.train()
    full_loss, full = _step_grads(m, px, lab)
    assert m.last_active_length == 60
    assert np.all((lab[:, 1:] != cfg.pad_id).sum(1) == 59)
    acc = torch.zeros_like(full)
    mean_loss = 0.0
    for i in range(16):
        sl = slice(16 * i, 16 * (i + 1))
        loss, g = _step_grads(m, px[sl], lab[sl])
        assert m.last_active_length == 60
        acc += g / 16
        mean_loss += loss / 16
    dl = abs(full_loss - mean_loss)
    worst = _rel_diff(cfg, full, acc)
    q = np.quantile(list(worst.values()), [0.5, 0.9, 0.99])
    print(f"decomposition: |dloss| {dl:.3g} (loss {full_loss:.5f}); gradients worst {max(worst.values()):.3g} "
          f"({max(worst, key=worst.get)}), median {q[0]:.3g}, 90 % {q[1]:.3g}, 99 % {q[2]:.3g}; one-dimensional tensors worst "
          f"{max(e for k, e in worst.items() if bench.sd[k].ndim == 1):.3g}")
    # self-check: image 100's share swapped for image 7 of another batch (same 59 targets, so the same weight 1/256)
    _, own = _step_grads(m, px[100:101], lab[100:101])
    _, other = _step_grads(m, px_o[7:8], lab_o[7:8])
    planted = full - own / 256 + other / 256
    share = _rel_diff(cfg, planted, acc)
    flagged = sum(e > DECOMP_MAX for e in share.values())
    ratio = sorted(e / DECOMP_MAX for e in share.values())
    print(f"decomposition self-check: one image's share flagged in {flagged} of {len(share)} tensors; share / bound: "
          f"min {ratio[0]:.3g}, 10 % {ratio[len(ratio) // 10]:.3g}, median {ratio[len(ratio) // 2]:.3g}")
    assert dl <= 5e-6 * full_loss
    _check_grads("decomposition", worst, DECOMP_MAX, DECOMP_MEDIAN)
    assert flagged == len(share), sorted(share.items(), key=lambda kv: kv[1])[:6]
