"""Class weights and the focal term of the training loss (include/kzv.h: kzv_set_class_weights, kzv_set_focal_gamma, kzv_ce_fwd_bwd_w,
kzv_target_weight_sum): the W instantiations of ce_kernel / ce_generic_kernel / head_ce_kernel (csrc/cross_entropy.hip) against float64
torch.  Over the scored rows i (target y_i != pad), p_ic = softmax(z_i)[c], p_i = p_i,y_i, nll_i = lse_i - z_i[y_i], W = sum_i w[y_i],
S_w = sum_c w[c]:

    gamma = 0:  F.cross_entropy(z, y, weight=w, ignore_index=pad, label_smoothing=eps)
                dlogits[i][c] = [((1 - eps) w[y_i] + (eps / V) S_w) p_ic - (1 - eps) w[y_i] [c == y_i] - (eps / V) w[c]] / W
    gamma > 0:  loss = sum_i w[y_i] (1 - p_i)^gamma nll_i / W                                  (eps = 0)
                dlogits[i][c] = w[y_i] g_i (p_ic - [c == y_i]) / W,   g_i = (1 - p_i)^gamma + gamma (1 - p_i)^(gamma - 1) p_i nll_i

Weights throughout are w = exp(U(-ln 4, ln 4)) from a seeded generator (a spread of 16).  What a wrong build would show: the count in
place of W, or a w[c] missing under eps, fails the operator test; an unguarded -(eps / V) w[c] / W in the padded columns or a read of w
past V fails the vocabulary-100 case of the head test; a missing clamp of nll gives NaN in the dominating-target test; weights or gamma
applied to evaluation forwards fail the eval test; a value lost between constructor, handle and checkpoint fails the round trip."""
import ctypes as C
import dataclasses
import math
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from kzv import _lib as L
from kzv import params as P
from kzv.config import micro_config, tiny_config
from kzv.data import build_decoder_dir, synthetic_batch
from kzv.model import TrOCRModel
from oracle import trocr_oracle as O

from _replay import step_masks

pytestmark = pytest.mark.gpu
DEV = "cuda"
PAD = 1
BF16_HALF_ULP = 2 ** -8      # |bf16(x) - x| <= 2^-8 |x|
HERE = os.path.dirname(os.path.abspath(__file__))
EMB = "decoder.roberta.embeddings.word_embeddings.weight"

# The operator's bounds, measured as tests/test_glue_ops_gpu.py and tests/test_label_smoothing_gpu.py measure theirs (the kernels use
# the fast exp / log, so the figures are read off an MI355X, not derived): the worst figure over the 20 cases of
# test_operator_against_float64 (4 vocabularies x the 5 configurations; each loss with and without a gradient buffer), times 4.  The
# margin of 4 is test_glue_ops_gpu.py's and for its reason: the rows' shares reach *loss by float atomics in no fixed order.
# Seven passes over the 20 cases (280 losses, in several processes) were read.  The losses are 10.5 .. 18.3 (one fp32 ulp of
# 16 is 1.9e-6) and move between passes by the order of the atomics: V 41, gamma 2, weights, with dlogits read 5.02e-7 in one pass,
# 3.36e-6 in the next and 1.46e-6 in four others; V 4300, gamma 0.5 read 5.49e-7 six times and 2.46e-6 once.  Every other loss was
# within 1.91e-6, the plain loss's own figure (CE_LOSS_MEASURED = 1.93e-6 in test_glue_ops_gpu.py).
# CE_W_FOCAL_C_MEASURED: the worst (|dlogits error| - 2^-8 |want|) / a_i over the real columns of the gamma > 0 cases, a_i = w[y_i] g_i / W
# the row's coefficient on the softmax.  It came out NEGATIVE in every case and every pass (between -1.4e-12 and -8e-18: every element
# lay inside its own bf16 rounding, the closest ones being softmax tails that round to tiny values), so nothing positive was measured and
# the bound is the floor the constant may not go below: max(4 x measured, 1e-6) = 1e-6, the gamma = 0 constant.
CE_W_LOSS_MEASURED = 3.36e-6       # V 41 (ce_kernel), eps 0, gamma 2, with weights, with dlogits
CE_W_LOSS_BOUND = 4 * CE_W_LOSS_MEASURED
CE_W_FOCAL_C_MEASURED = 0.0        # no gamma > 0 case left its bf16 rounding term: the largest excess read was -8e-18 a_i (V 4300, gamma 2, no weights)
CE_W_FOCAL_C = max(4 * CE_W_FOCAL_C_MEASURED, 1e-6)
CE_W_C = 1e-6                      # gamma = 0: the existing 2^-8 |want| + 1e-6 / n with 1 / n generalised to the row's coefficient

CONFIGS = [(0.0, 0.0, True), (0.1, 0.0, True), (0.0, 2.0, True), (0.0, 0.5, True), (0.0, 2.0, False)]      # (eps, gamma, weights)
SHAPES = [(41, 64), (777, 832), (4300, 4352), (5121, 5184)]                                              # the last: ce_generic_kernel


@pytest.fixture(scope="module")
def lib():
    return L.load()


@pytest.fixture(autouse=True)
def _default_head_mode_afterwards():
    yield
    L.load().kzv_set_head_ce(-1)


def _st():
    return torch.cuda.current_stream().cuda_stream


def _weights(V, seed=0, device=DEV):
    """w = exp(U(-ln 4, ln 4)), fp32 [V], seeded."""
    g = torch.Generator(device="cpu").manual_seed(1000 + V + seed)
    u = torch.rand(V, generator=g, dtype=torch.float64) * 2 - 1
    return torch.exp(u * math.log(4.0)).float().to(device)


def stated_loss(x, tgt, w, eps, gamma, pad=PAD):
    """The module docstring's loss in torch on x [rows, V] (any float dtype, autograd flows), w [V] or None.  Returns (loss, a) with a the
    rows' coefficients on the softmax (detached; 0 in pad rows)."""
    V = x.shape[1]
    live = tgt != pad
    ww = torch.ones(V, dtype=x.dtype, device=x.device) if w is None else w.to(x.dtype)
    wy = ww[tgt.clamp(0, V - 1)] * live
    Wn = wy.sum()
    if gamma == 0:
        loss = F.cross_entropy(x, tgt, weight=None if w is None else ww, ignore_index=pad, label_smoothing=eps)
        a = ((1 - eps) * wy + eps / V * ww.sum() * live) / Wn
        return loss, a.detach()
    assert eps == 0
    logp = torch.log_softmax(x, 1)
    nll = -logp.gather(1, tgt.clamp(0, V - 1)[:, None])[:, 0]
    p = torch.exp(-nll)
    loss = (wy * (1 - p) ** gamma * nll).sum() / Wn
    g = (1 - p) ** gamma + gamma * (1 - p) ** (gamma - 1) * p * nll
    return loss, (wy * g / Wn).detach()


@pytest.fixture(scope="module")
def op_cases():
    """The inputs of tests/test_label_smoothing_gpu.py::test_operator_against_float64 (B 3, T 7, label stride 16, randn * 4, columns
    [V, ldl) filled with +50, the same pad pattern), one per shape, with the weights; built once and left unchanged."""
    out = {}
    B, T, L_ = 3, 7, 16
    for V, ldl in SHAPES:
        gen = torch.Generator(device=DEV).manual_seed(V)
        logits = torch.randn(B * T, ldl, device=DEV, generator=gen) * 4
        logits[:, V:] = 50.0
        lab = torch.randint(2, V, (B, L_), device=DEV, generator=gen, dtype=torch.int64)
        lab[0, 5:] = PAD
        lab[1, :] = PAD
        lab[2, 7] = PAD
        tgt = lab[:, 1:T + 1].reshape(-1)
        out[V] = dict(B=B, T=T, L=L_, V=V, ldl=ldl, logits=logits, lab=lab, tgt=tgt, live=tgt != PAD, w=_weights(V))
    return out


def _norm2(lib, c, w):
    out = torch.full((2,), float("nan"), device=DEV)
    L.check(lib.kzv_target_weight_sum(c["lab"].data_ptr(), c["L"], c["B"], c["T"], c["V"], PAD, L.ptr(w), out.data_ptr(), _st()), "target_weight_sum")
    torch.cuda.synchronize()
    return out


def _call(lib, c, norm2, eps, gamma, w, with_grad=True, entry="w"):
    loss = torch.zeros(1, device=DEV)
    dl = torch.full((c["B"] * c["T"], c["ldl"]), float("nan"), dtype=torch.bfloat16, device=DEV) if with_grad else None
    a = (c["logits"].data_ptr(), c["ldl"], c["lab"].data_ptr(), c["L"], c["B"], c["T"], c["V"], PAD, norm2.data_ptr(), loss.data_ptr(), L.ptr(dl))
    if entry == "w":
        rc = lib.kzv_ce_fwd_bwd_w(*a, eps, L.ptr(w), gamma, _st())
    else:
        rc = lib.kzv_ce_fwd_bwd_ls(*a, eps, _st())
    L.check(rc, "ce_fwd_bwd")
    torch.cuda.synchronize()
    return float(loss), dl


def _reference(c, w, eps, gamma):
    x = c["logits"][:, :c["V"]].double().requires_grad_(True)
    ref, a = stated_loss(x, c["tgt"], None if w is None else w.double(), eps, gamma)
    ref.backward()
    want = torch.zeros(c["B"] * c["T"], c["ldl"], dtype=torch.float64, device=DEV)
    want[:, :c["V"]] = x.grad
    assert bool((want[~c["live"]] == 0).all())
    return float(ref.detach()), want, a


def _check_dlogits(c, dl, want, a, cc):
    """pad rows and columns >= V exactly zero; every other element within 2^-8 |want| + cc a_i.  Returns the worst (|err| - 2^-8 |want|) / a_i
    over the real columns of the scored rows (negative: inside the bf16 rounding) and the number of elements outside the bound."""
    live, V = c["live"], c["V"]
    assert bool((dl[~live] == 0).all()) and bool((dl[:, V:] == 0).all())
    err = torch.nan_to_num((dl.double() - want).abs(), nan=float("inf"))
    excess = ((err - BF16_HALF_ULP * want.abs())[live][:, :V] / a[live][:, None]).max()
    tol = BF16_HALF_ULP * want.abs() + cc * a[:, None]
    bad = ~(err <= tol)
    return float(excess), int(bad.sum())


# ================================================================================================ 1. the operator
@pytest.mark.parametrize("eps,gamma,weighted", CONFIGS)
@pytest.mark.parametrize("V,ldl", SHAPES)
def test_operator_against_float64(lib, op_cases, V, ldl, eps, gamma, weighted):
    """kzv_ce_fwd_bwd_w on the label-smoothing operator test's inputs; norm2 from kzv_target_weight_sum (within 1e-6 relative of the
    float64 sums, two calls bit-equal).  Reference: float64 F.cross_entropy(weight, label_smoothing) for gamma 0, the focal formula of the
    module docstring in torch for gamma > 0, both under autograd on the same fp32 logits.  dlogits: pad-target rows and columns [V, ldl)
    exactly zero, every other element within 2^-8 |want| + c a_i (a_i: the row's coefficient on the softmax; c = 1e-6 for gamma 0,
    CE_W_FOCAL_C for gamma > 0); loss within CE_W_LOSS_BOUND with and without a gradient buffer.
    Measured on an MI355X: see CE_W_LOSS_MEASURED / CE_W_FOCAL_C_MEASURED."""
    c = op_cases[V]
    w = c["w"] if weighted else None
    norm2 = _norm2(lib, c, w)
    assert torch.equal(norm2, _norm2(lib, c, w))
    ww = torch.ones(V, dtype=torch.float64, device=DEV) if w is None else w.double()
    want_W, want_S = float(ww[c["tgt"][c["live"]]].sum()), float(ww.sum())
    assert abs(float(norm2[0]) - want_W) <= 1e-6 * want_W and abs(float(norm2[1]) - want_S) <= 1e-6 * want_S
    want_loss, want, a = _reference(c, w, eps, gamma)
    losses = []
    for with_grad in (True, False):
        lv, dl = _call(lib, c, norm2, eps, gamma, w, with_grad)
        losses.append(lv)
        if with_grad:
            excess, nbad = _check_dlogits(c, dl, want, a, CE_W_FOCAL_C if gamma > 0 else CE_W_C)
    errs = [abs(v - want_loss) for v in losses]
    print(f"ce_w V {V} ldl {ldl} eps {eps} gamma {gamma} weights {weighted}: loss {losses[0]:.7f} (float64 {want_loss:.7f}), |error| {errs[0]:.3g} with "
          f"dlogits, {errs[1]:.3g} without; worst (|dlogits error| - 2^-8 |want|) / a_i = {excess:.3g}")
    assert nbad == 0, f"{nbad} dlogits outside the bound, worst excess {excess:.3g} a_i"
    assert max(errs) <= CE_W_LOSS_BOUND, (errs, CE_W_LOSS_BOUND)


# ================================================================================================ 2. a target that dominates
@pytest.mark.parametrize("gamma", [0.5, 2.0])
def test_dominating_target_stays_finite(lib, gamma):
    """V 41, one scored row whose target logit lies 30 above every other.  1 - p is then about 40 e^-30, far below what fp32 lse - z_y
    resolves (delta <= 1e-5), and lse - z_y may come out below zero: without the clamp the fractional power is NaN.  With it
    g_i |p - onehot| <= (1 + gamma) delta^(1 + gamma) <= 5e-8, so every |dlogits| of the row is at most 1e-6 w[y] / W."""
    V, ldl = 41, 64
    gen = torch.Generator(device=DEV).manual_seed(7)
    logits = torch.randn(1, ldl, device=DEV, generator=gen) * 4
    y = 17
    logits[0, y] = float(logits[0, :V].max()) + 30.0
    logits[0, V:] = 50.0
    lab = torch.tensor([[2, y, PAD, PAD]], dtype=torch.int64, device=DEV)
    w = _weights(V)
    c = dict(B=1, T=1, L=4, V=V, ldl=ldl, logits=logits, lab=lab)
    norm2 = _norm2(lib, c, w)
    assert float(norm2[0]) == float(w[y])
    loss, dl = _call(lib, c, norm2, 0.0, gamma, w)
    print(f"dominating target, gamma {gamma}: loss {loss:.3g}, largest |dlogits| {float(dl.float().abs().max()):.3g}")
    assert math.isfinite(loss) and loss >= 0 and bool(torch.isfinite(dl.float()).all())
    assert float(dl.float().abs().max()) <= 1e-6 * float(w[y]) / float(norm2[0])
    assert bool((dl[:, V:] == 0).all())


# ================================================================================================ 3. off is the code that runs today
@pytest.mark.parametrize("V,ldl", SHAPES)
def test_off_is_todays_kernels_and_the_scale_of_the_weights_cancels(lib, op_cases, V, ldl):
    """kzv_ce_fwd_bwd_w(..., NULL, 0) at eps 0 and 0.1 gives kzv_ce_fwd_bwd_ls's dlogits bit for bit (norm2[0] acting as count); constant
    weights w = 3 give the loss and dlogits of w = 1 within the bounds of the operator test (the loss does not see the scale of w)."""
    c = op_cases[V]
    n = int(c["live"].sum())
    norm2 = _norm2(lib, c, None)
    assert float(norm2[0]) == n and float(norm2[1]) == V
    for eps in (0.0, 0.1):
        _, d0 = _call(lib, c, norm2, eps, 0.0, None)
        _, d1 = _call(lib, c, norm2, eps, 0.0, None, entry="ls")
        assert torch.equal(d0, d1)
    w3 = torch.full((V,), 3.0, device=DEV)
    n3 = _norm2(lib, c, w3)
    assert float(n3[0]) == 3.0 * n and abs(float(n3[1]) - 3.0 * V) <= 1e-6 * 3.0 * V
    for eps in (0.0, 0.1):
        want_loss, want, a = _reference(c, None, eps, 0.0)
        loss, dl = _call(lib, c, n3, eps, 0.0, w3)
        excess, nbad = _check_dlogits(c, dl, want, a, CE_W_C)
        assert nbad == 0 and abs(loss - want_loss) <= CE_W_LOSS_BOUND, (nbad, excess, loss, want_loss)


# ================================================================================================ the model cases
def _head_cfg(vocab=None):
    kw = {} if vocab is None else {"vocab": vocab}
    return dataclasses.replace(tiny_config(), dec_hidden=256, dec_heads=4, dec_ffn=768, dec_layers=2, **kw)


def _model(cfg, tmp_path, seed, **kw):
    d = build_decoder_dir(str(tmp_path / f"dec{cfg.vocab}"), cfg)
    return TrOCRModel(cfg.encoder_config_dict(), d, init_seed=seed, load_tokenizer=False, **kw)


MODEL_CONFIGS = [(True, 0.1, 0.0), (True, 0.0, 2.0), (False, 0.0, 2.0)]      # (weights, eps, gamma)


@pytest.mark.parametrize("weighted,eps,gamma", MODEL_CONFIGS)
@pytest.mark.parametrize("B,Lh,vocab", [(5, 30, 4300), (3, 12, 100), (70, 9, 4300)])
def test_one_launch_head_equals_gemm_plus_ce(tmp_path, B, Lh, vocab, weighted, eps, gamma):
    """tests/test_label_smoothing_gpu.py's head test under weights / focal: kzv_set_head_ce(0) (head GEMM + ce_kernel<false, true>) against
    (1) (head_ce_kernel<*, false, true>), same model, batch and dropout seed.  Loss within 2e-6 relative, every gradient within 2e-3 of the
    largest.  Vocabulary 100 (Vp 128) ends inside a chunk and inside a pad: an unguarded -(eps / V) w[c] / W in columns [100, 128), or a
    read of w past V, shows up there."""
    cfg = _head_cfg(vocab)
    lib = L.load()
    m = _model(cfg, tmp_path, 3 + B, label_smoothing=eps, focal_gamma=gamma, class_weights=_weights(vocab, device="cpu") if weighted else None)
    px, lab = synthetic_batch(cfg, B, Lh, seed=5 + B, min_chars=1, max_chars=Lh - 2)
    pxt, ids = torch.from_numpy(px).cuda(), torch.from_numpy(lab).cuda()
    out = []
    for mode in (0, 1):
        L.check(lib.kzv_set_head_ce(mode), "mode")
        m.train()
        m.zero_grad()
        loss, _ = m.forward_loss(pxt, ids, want_logits=False, seed=13)
        m.backward()
        torch.cuda.synchronize()
        out.append((float(loss), m.flat_grads.clone()))
    (l0, g0), (l1, g1) = out
    dg = float((g0 - g1).abs().max()); sc = float(g0.abs().max())
    print(f"B={B} L={Lh} V={vocab} weights {weighted} eps {eps} gamma {gamma}: loss {l0:.6f} / {l1:.6f}, largest gradient difference {dg:.2e} of {sc:.2e}")
    assert np.isfinite(l1) and abs(l0 - l1) < 2e-6 * max(1.0, abs(l0)), (l0, l1)
    assert bool(torch.isfinite(g1).all()) and dg < 2e-3 * sc


@pytest.mark.parametrize("weighted,eps,gamma", MODEL_CONFIGS)
@pytest.mark.parametrize("B,Lh,vocab", [(5, 30, 4300), (3, 12, 100)])
def test_fused_loss_is_the_stated_loss_on_the_same_logits(tmp_path, B, Lh, vocab, weighted, eps, gamma):
    """Train mode, fixed dropout seed, the full decoder length on both calls: the fp32 logits of forward_loss(want_logits=True) under the
    float64 statement against the fused loss of want_logits=False (and the materialised one that came with the logits).  Bound: the
    operator's measured loss bound + 1e-5 relative."""
    cfg = _head_cfg(vocab)
    w = _weights(vocab, device="cpu") if weighted else None
    m = _model(cfg, tmp_path, 3 + B, label_smoothing=eps, focal_gamma=gamma, class_weights=w)
    m.trim_padding = False
    px, lab = synthetic_batch(cfg, B, Lh, seed=5 + B, min_chars=1, max_chars=Lh - 2)
    pxt, ids = torch.from_numpy(px).cuda(), torch.from_numpy(lab).cuda()
    m.train()
    loss_m, logits = m.forward_loss(pxt, ids, want_logits=True, seed=13)
    loss_m = float(loss_m)
    loss_f = float(m.forward_loss(pxt, ids, want_logits=False, seed=13)[0])
    tgt = ids[:, 1:].reshape(-1)
    x = logits.reshape(-1, vocab).double()
    want = float(stated_loss(x, tgt, None if w is None else w.cuda().double(), eps, gamma, cfg.pad_id)[0])
    plain = float(F.cross_entropy(x, tgt, ignore_index=cfg.pad_id))
    tol = CE_W_LOSS_BOUND + 1e-5 * abs(want)
    print(f"B={B} L={Lh} V={vocab} weights {weighted} eps {eps} gamma {gamma}: fused {loss_f:.7f}, materialised {loss_m:.7f}, float64 {want:.7f} "
          f"(plain {plain:.7f}); bound {tol:.3g}")
    assert abs(loss_f - want) <= tol and abs(loss_m - want) <= tol


def test_eval_mode_ignores_weights_and_gamma(tmp_path):
    """(7, 23, 777), m.eval(): with weights and gamma 2 set, the loss is the float64 PLAIN cross-entropy of the returned logits, on the fused
    and on the materialised path, and equals the loss with neither set within 2e-6 relative.  The tied embedding / head weight is scaled by
    16 first (test_label_smoothing_gpu.py's trick), so that the plain, the weighted and the focal loss of the batch differ by far more
    than the bound (asserted)."""
    B, Lh, vocab = 7, 23, 777
    cfg = _head_cfg(vocab)
    m = _model(cfg, tmp_path, 3 + B)
    m.state_dict_views()[EMB].mul_(16.0)      # before the first bind, which casts the weights
    px, lab = synthetic_batch(cfg, B, Lh, seed=5 + B, min_chars=1, max_chars=Lh - 2)
    pxt, ids = torch.from_numpy(px).cuda(), torch.from_numpy(lab).cuda()
    w = _weights(vocab, device="cpu")
    m.eval()
    got = {}
    for on in (True, False):
        m.class_weights = w if on else None
        m.focal_gamma = 2.0 if on else 0.0
        assert (m.class_weights is not None) == on and m.focal_gamma == (2.0 if on else 0.0)
        lf = float(m.forward_loss(pxt, ids, want_logits=False)[0])
        lm, logits = m.forward_loss(pxt, ids, want_logits=True)
        got[on] = (lf, float(lm), logits.clone())
    assert torch.equal(got[True][2], got[False][2])
    tgt = ids[:, 1:].reshape(-1)
    x = got[False][2].reshape(-1, vocab).double()
    want = float(F.cross_entropy(x, tgt, ignore_index=cfg.pad_id))
    weighted = float(stated_loss(x, tgt, w.cuda().double(), 0.0, 0.0, cfg.pad_id)[0])
    focal = float(stated_loss(x, tgt, w.cuda().double(), 0.0, 2.0, cfg.pad_id)[0])
    tol = CE_W_LOSS_BOUND + 1e-5 * abs(want)
    print(f"eval: fused {got[True][0]:.7f} / {got[False][0]:.7f}, materialised {got[True][1]:.7f} / {got[False][1]:.7f}, float64 plain {want:.7f} "
          f"(weighted {weighted:.7f}, weighted focal {focal:.7f})")
    assert abs(weighted - want) > 100 * tol and abs(focal - want) > 100 * tol
    for i in (0, 1):
        assert abs(got[True][i] - got[False][i]) < 2e-6 * max(1.0, abs(got[False][i]))
        assert abs(got[True][i] - want) <= tol and abs(got[False][i] - want) <= tol


# ================================================================================================ 7. the whole step
@pytest.mark.parametrize("fused,weighted,gamma", [(False, True, 0.0), (True, True, 0.0), (True, False, 2.0)],
                         ids=["weights-materialised", "weights-one-launch-head", "focal-one-launch-head"])
def test_whole_step_against_the_oracle_with_the_stated_loss(tmp_path, fused, weighted, gamma):
    """test_parity_gpu.py::_replay_case under weights / focal, dropout on: the oracle's network (O.forward with the step's own masks) gives
    the logits, the test applies the stated loss and calls backward.  tiny_config takes head GEMM + ce_kernel, the 256 / 4 / 768 decoder
    the one-launch head.  That function's metric and tolerances: per tensor max|have - want| / max|want| <= 0.05, loss within 5e-3,
    key.bias skipped.  The guard, from the oracle alone: the plain-loss gradient of decoder.lm_head.bias misses the weighted (resp. focal)
    one by more than that tolerance, so an engine that ignored the setting could not pass.
    The focal case needs targets the model already predicts: at the recipe's flat initial logits every p_i is about 1 / V, every g_i about
    1, and the focal gradient IS the plain one.  So half the targets are made one class K, and lm_head.bias[K] (a parameter of its own,
    changed alike in the model and in the oracle's leaves) is raised to ln V + 1: p_K is then about 0.73 in every row, g_i about 0.2 in
    the rows whose target is K and about 1 in the others."""
    grad_tol, B, Lh, seed, model_seed, K = 0.05, 3, 24, 12345, 42, 9
    cfg = dataclasses.replace(tiny_config(), dec_hidden=256, dec_heads=4, dec_ffn=768) if fused else tiny_config()
    w = _weights(cfg.vocab, device="cpu") if weighted else None
    m = _model(cfg, tmp_path, model_seed, class_weights=w, focal_gamma=gamma)
    m.trim_padding = False                      # the masks below are drawn for the full decoder length
    px, lab = synthetic_batch(cfg, B, Lh, seed=3, min_chars=3, max_chars=Lh - 1)
    flat = P.recipe_flat(cfg, model_seed)
    sd = P.state_dict_from_flat(cfg, flat)
    if gamma > 0:
        lab[:, 1::2] = np.where(lab[:, 1::2] != cfg.pad_id, K, cfg.pad_id)
        sd["decoder.lm_head.bias"][K] = math.log(cfg.vocab) + 1.0
        m.state_dict_views()["decoder.lm_head.bias"][K] = math.log(cfg.vocab) + 1.0      # before the first bind
    m.train()
    m.zero_grad()
    loss, _ = m.forward_loss(torch.from_numpy(px), torch.from_numpy(lab), want_logits=False, seed=seed)
    m.backward()
    torch.cuda.synchronize()
    masks = step_masks(cfg, seed, B, Lh - 1)
    assert len(masks) == 1 + 3 * cfg.enc_layers + 1 + 5 * cfg.dec_layers
    leaves = O.leaf_state_dict(sd)
    labt = torch.from_numpy(lab)
    logits, plain = O.forward(cfg, leaves, torch.from_numpy(px), labt, masks=masks)
    want_loss, _ = stated_loss(logits.reshape(-1, logits.shape[-1]), labt[:, 1:].reshape(-1), w, 0.0, gamma, cfg.pad_id)
    bias = leaves["decoder.lm_head.bias"]
    g_plain = torch.autograd.grad(plain, bias, retain_graph=True)[0]
    want_loss.backward()
    miss = float((g_plain - bias.grad).abs().max() / (bias.grad.abs().max() + 1e-9))
    want_loss = want_loss.detach()
    print(f"oracle: loss {float(want_loss):.5f} stated / {float(plain.detach()):.5f} plain; lm_head.bias gradient of the plain loss misses by {miss:.3g}")
    assert miss > grad_tol
    assert abs(float(loss.item()) - float(want_loss)) < 5e-3
    g = m.grad_dict()
    worst = {}
    for k, leaf in leaves.items():
        if leaf.grad is None or k.endswith("key.bias"):      # exactly-zero true gradient (softmax shift invariance)
            continue
        want = leaf.grad.numpy()
        have = g[k].cpu().numpy().reshape(want.shape)
        worst[k] = float(np.abs(have - want).max() / (np.abs(want).max() + 1e-9))
    bad = {k: e for k, e in worst.items() if e > grad_tol}
    print(f"worst relative gradient error {max(worst.values()):.4g}, median {np.median(list(worst.values())):.4g}, dloss {abs(float(loss.item()) - float(want_loss)):.3g}")
    assert not bad, sorted(bad.items(), key=lambda kv: -kv[1])[:8]


# ================================================================================================ 8. ranges and round trip
def test_ranges_and_checkpoint_round_trip(tmp_path, lib):
    from kzv.trainer import load_checkpoint, save_checkpoint
    cfg = micro_config()
    V = cfg.vocab
    d = build_decoder_dir(str(tmp_path / "dec"), cfg)
    golden = os.path.join(HERE, "golden", "micro_lightning.ckpt")
    enc = torch.load(golden, map_location="cpu", weights_only=False)["hyper_parameters"]["encoder_config"]
    m = TrOCRModel(enc, d, init_seed=1, load_tokenizer=False)
    buf = (C.c_float * V)()

    def handle_weights():
        n = lib.kzv_get_class_weights(m._h, buf, V)
        return None if n == 0 else torch.tensor(list(buf[:n]))

    assert m.class_weights is None and m.focal_gamma == 0.0 and handle_weights() is None and lib.kzv_get_focal_gamma(m._h) == 0.0
    assert m.hparams.class_weights is None and m.hparams.focal_gamma == 0.0
    w = _weights(V, device="cpu")
    m.class_weights = w
    m.focal_gamma = 1.5
    assert torch.equal(m.class_weights, w) and torch.equal(handle_weights(), w) and lib.kzv_get_focal_gamma(m._h) == 1.5
    # refused at the ABI with -1 (KZV_E_ARG), the previous state left in place ...
    arr = lambda t: (C.c_float * len(t))(*[float(v) for v in t])      # noqa: E731
    for bad in (w[:-1], torch.cat([w, w[:1]])):
        assert lib.kzv_set_class_weights(m._h, arr(bad), len(bad)) == -1
    for v in (0.0, -1.0, float("nan"), float("inf")):
        b = w.clone(); b[3] = v
        assert lib.kzv_set_class_weights(m._h, arr(b), V) == -1
    for gbad in (-0.1, 5.1, float("nan")):
        assert lib.kzv_set_focal_gamma(m._h, gbad) == -1
    assert lib.kzv_set_label_smoothing(m._h, 0.1) == -1                  # gamma 1.5 is set: eps > 0 refused
    assert torch.equal(handle_weights(), w) and lib.kzv_get_focal_gamma(m._h) == 1.5 and lib.kzv_get_label_smoothing(m._h) == 0.0
    # ... and in Python with ValueError
    for bad in (w[:-1], torch.cat([w, w[:1]]), [1.0] * (V - 1)):
        with pytest.raises(ValueError):
            m.class_weights = bad
    for v in (0.0, -1.0, float("nan"), float("inf")):
        b = w.clone(); b[3] = v
        with pytest.raises(ValueError):
            m.class_weights = b
        with pytest.raises(ValueError):
            TrOCRModel(enc, d, init_seed=1, load_tokenizer=False, class_weights=b)
    for gbad in (-0.1, 5.1, float("nan")):
        with pytest.raises(ValueError):
            m.focal_gamma = gbad
        with pytest.raises(ValueError):
            TrOCRModel(enc, d, init_seed=1, load_tokenizer=False, focal_gamma=gbad)
    with pytest.raises(ValueError):
        m.label_smoothing = 0.1
    with pytest.raises(ValueError):
        TrOCRModel(enc, d, init_seed=1, load_tokenizer=False, focal_gamma=2.0, label_smoothing=0.1)
    assert torch.equal(m.class_weights, w) and m.focal_gamma == 1.5 and m.label_smoothing == 0.0
    # the reverse order
    m.focal_gamma = 0.0
    m.label_smoothing = 0.1
    assert lib.kzv_set_focal_gamma(m._h, 2.0) == -1
    with pytest.raises(ValueError):
        m.focal_gamma = 2.0
    assert m.focal_gamma == 0.0 and lib.kzv_get_focal_gamma(m._h) == 0.0 and m.label_smoothing == 0.1
    m.label_smoothing = 0.0
    m.focal_gamma = 1.5
    # the operator refuses them too
    z = torch.zeros(1, 8, device=DEV); lab = torch.full((1, 2), 2, dtype=torch.int64, device=DEV); one = torch.ones(2, device=DEV)
    for e, gbad in ((0.0, -0.1), (0.0, 5.1), (0.0, float("nan")), (0.1, 2.0)):
        assert lib.kzv_ce_fwd_bwd_w(z.data_ptr(), 8, lab.data_ptr(), 2, 1, 1, 8, PAD, one.data_ptr(), one.data_ptr(), None, e, None, gbad, _st()) == -1
    # lists and arrays are taken as well
    m.class_weights = w.tolist()
    assert torch.equal(m.class_weights, w)
    m.class_weights = w.numpy()
    assert torch.equal(m.class_weights, w) and m.class_weights.dtype == torch.float32
    # round trip
    path = tmp_path / "weighted.ckpt"
    save_checkpoint(m, None, str(path), 0, 1)
    hp = torch.load(path, map_location="cpu", weights_only=False)["hyper_parameters"]
    assert torch.equal(hp["class_weights"], w) and hp["class_weights"].dtype == torch.float32 and hp["focal_gamma"] == 1.5
    m2 = TrOCRModel(enc, d, init_seed=2, load_tokenizer=False)
    load_checkpoint(m2, None, str(path))
    n = lib.kzv_get_class_weights(m2._h, buf, V)
    assert n == V and torch.equal(torch.tensor(list(buf[:n])), w)
    assert torch.equal(m2.class_weights, w) and m2.focal_gamma == 1.5 and lib.kzv_get_focal_gamma(m2._h) == 1.5
    assert torch.equal(m2.flat_params, m.flat_params)
    # a reference checkpoint has no such keys: the plain loss
    load_checkpoint(m2, None, golden)
    assert m2.class_weights is None and m2.focal_gamma == 0.0
    assert lib.kzv_get_class_weights(m2._h, buf, V) == 0 and lib.kzv_get_focal_gamma(m2._h) == 0.0
    # clearing
    m.class_weights = None
    assert m.class_weights is None and lib.kzv_get_class_weights(m._h, buf, V) == 0
