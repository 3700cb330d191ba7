"""Label smoothing of the training loss (include/kzv.h: kzv_set_label_smoothing, kzv_ce_fwd_bwd_ls): the three loss kernels' LS
instantiations -- ce_kernel / ce_generic_kernel and the one-launch head_ce_kernel (all three: csrc/cross_entropy.hip) -- against
torch.nn.functional.cross_entropy(logits, target, ignore_index=pad, label_smoothing=eps), mean over the scored rows, V = the real vocabulary:

    loss_row   = lse(z) - (1 - eps) z[y] - (eps / V) sum_{v < V} z[v]
    dlogits[v] = (softmax(z)[v] - (1 - eps) [v == y] - eps / V) / count   for v < V,   0 for V <= v < Vp

What a wrong build would show: Vp in place of V, or a missing guard of the padded columns (they would hold -eps / (V count) instead of zero and
enter the head's gradient GEMMs), fails the operator test and the vocabulary-100 case of the head test; smoothing applied to evaluation
forwards fails the eval test; a value lost between constructor, handle and checkpoint fails the round trip."""
import dataclasses
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

# Loss bound of the operator: the kernels use the fast exp / log, so the bound is measured, not derived (as tests/test_glue_ops_gpu.py does
# for the plain loss): 4 x the worst |loss - float64 loss| over the 16 calls below (4 vocabularies x eps 0.1 / 0.3 x with / without dlogits)
# on an MI355X, the worst of two runs of the file (32 losses).  The margin of 4 is that test's and for its reason: the rows' shares reach
# *loss by float atomics in no fixed order, which moves the last ulp of the sum from run to run (V 5121, eps 0.3, with dlogits: 1.59e-6 in
# one run, 3.2e-7 in the other).  The losses here are 10.2 .. 17.6 (one fp32 ulp of 16 is 1.9e-6).  The figure lies below the plain
# loss's 1.93e-6 (CE_LOSS_MEASURED there): the two extra terms add no visible error.
CE_LS_LOSS_MEASURED = 1.59e-6      # V 5121 (ce_generic_kernel), eps 0.3, with dlogits; 1.55e-6 at V 4300 eps 0.3 in both runs; every other loss <= 1.29e-6
CE_LS_LOSS_BOUND = 4 * CE_LS_LOSS_MEASURED


@pytest.fixture(scope="module")
def lib():
    return L.load()


@pytest.fixture(autouse=True)
def _default_head_mode_afterwards():
    yield
    L.load().kzv_set_head_ce(-1)


def _st():
    return torch.cuda.current_stream().cuda_stream


def _ce64(logits, tgt, eps, pad=PAD):
    """float64 F.cross_entropy of fp32 logits [rows, V]."""
    return float(F.cross_entropy(logits.double(), tgt, ignore_index=pad, label_smoothing=eps))


# ================================================================================================ 1. the operator
@pytest.mark.parametrize("eps", [0.1, 0.3])
@pytest.mark.parametrize("V,ldl", [(41, 64), (777, 832), (4300, 4352), (5121, 5184)])
def test_operator_against_float64(lib, V, ldl, eps):
    """kzv_ce_fwd_bwd_ls with the shapes and inputs of test_glue_ops_gpu.py::test_cross_entropy_fwd_bwd (B 3, T 7, label stride 16, logits
    randn * 4, columns [V, ldl) filled with +50, the same pad pattern); ldl 5184 takes ce_generic_kernel.  Reference: float64 F.cross_entropy
    with label_smoothing and its autograd gradient on the same fp32 logits.  dlogits: pad-target rows and columns [V, ldl) exactly zero, every
    other element within 2^-8 |want| + 1e-6 / n (one bf16 rounding + the fp32 softmax); loss within CE_LS_LOSS_BOUND with and without a
    gradient buffer.  eps = 0 through this entry point gives kzv_ce_fwd_bwd's dlogits bit for bit."""
    B, T, L_ = 3, 7, 16
    gen = torch.Generator(device=DEV).manual_seed(V)
    logits = torch.randn(B * T, ldl, device=DEV, generator=gen) * 4
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
    x = logits[:, :V].double().requires_grad_(True)
    ref = F.cross_entropy(x, tgt, ignore_index=PAD, label_smoothing=eps)
    ref.backward()
    want_loss = float(ref.detach())
    want = torch.zeros(B * T, ldl, dtype=torch.float64, device=DEV)
    want[:, :V] = x.grad
    assert bool((want[~live] == 0).all())
    # torch's loss is the formula of the module docstring (V, not ldl, under eps)
    lse = torch.logsumexp(x.detach(), 1)
    rows = lse - (1 - eps) * x.detach().gather(1, tgt[:, None])[:, 0] - eps / V * x.detach().sum(1)
    assert abs(float((rows * live).sum() / n) - want_loss) < 1e-12 * abs(want_loss)

    def call(e, with_grad, entry="ls"):
        loss = torch.zeros(1, device=DEV)
        dl = torch.full((B * T, ldl), float("nan"), dtype=torch.bfloat16, device=DEV) if with_grad else None
        if entry == "ls":
            rc = lib.kzv_ce_fwd_bwd_ls(logits.data_ptr(), ldl, lab.data_ptr(), L_, B, T, V, PAD, count.data_ptr(), loss.data_ptr(), L.ptr(dl), e, _st())
        else:
            rc = lib.kzv_ce_fwd_bwd(logits.data_ptr(), ldl, lab.data_ptr(), L_, B, T, V, PAD, count.data_ptr(), loss.data_ptr(), L.ptr(dl), _st())
        L.check(rc, "ce_fwd_bwd")
        torch.cuda.synchronize()
        return float(loss), dl

    losses = []
    for with_grad in (True, False):
        lv, dl = call(eps, with_grad)
        losses.append(lv)
        if with_grad:
            assert bool((dl[~live] == 0).all()) and bool((dl[:, V:] == 0).all())
            err = (dl.double() - want).abs()
            err = torch.nan_to_num(err, nan=float("inf"))
            tol = BF16_HALF_ULP * want.abs() + 1e-6 / n
            bad = ~(err <= tol)
            assert not bool(bad.any()), f"{int(bad.sum())} dlogits outside the bound, worst ratio {float((err / tol).max()):.3g}"
    errs = [abs(v - want_loss) for v in losses]
    print(f"ce_ls V {V} ldl {ldl} eps {eps}: loss {losses[0]:.7f} (float64 {want_loss:.7f}), |error| {errs[0]:.3g} with dlogits, {errs[1]:.3g} without")
    assert max(errs) <= CE_LS_LOSS_BOUND, (errs, CE_LS_LOSS_BOUND)
    if eps == 0.1:       # once per shape: eps = 0 is the plain kernel
        _, d0 = call(0.0, True)
        _, d1 = call(0.0, True, entry="plain")
        assert torch.equal(d0, d1)


# ================================================================================================ the model cases
def _head_cfg(vocab=None):
    kw = {} if vocab is None else {"vocab": vocab}
    return dataclasses.replace(tiny_config(), dec_hidden=256, dec_heads=4, dec_ffn=768, dec_layers=2, **kw)


def _model(cfg, tmp_path, seed, **kw):
    d = build_decoder_dir(str(tmp_path / f"dec{cfg.vocab}"), cfg)
    return TrOCRModel(cfg.encoder_config_dict(), d, init_seed=seed, load_tokenizer=False, **kw)


@pytest.mark.parametrize("B,Lh,vocab", [(5, 30, 4300), (3, 12, 100), (70, 9, 4300)])
def test_one_launch_head_equals_gemm_plus_ce_under_smoothing(tmp_path, B, Lh, vocab):
    """test_decoder_chain_gpu.py's head test in train mode with eps 0.1: kzv_set_head_ce(0) (head GEMM + ce_kernel<true>) against (1)
    (head_ce_kernel<*, true>), same model, batch and dropout seed.  Loss within 2e-6 relative, every gradient within 2e-3 of the largest
    (bf16 dlogits on both sides).  Vocabulary 100 (Vp 128) ends inside a chunk and inside a pad: an unguarded -eps / V in columns
    [100, 128) would reach the head's weight gradient and dh."""
    cfg = _head_cfg(vocab)
    lib = L.load()
    m = _model(cfg, tmp_path, 3 + B, label_smoothing=0.1)
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
    print(f"B={B} L={Lh} V={vocab} eps 0.1: loss {l0:.6f} / {l1:.6f}, largest gradient difference {dg:.2e} of {sc:.2e}")
    assert np.isfinite(l1) and abs(l0 - l1) < 2e-6 * max(1.0, abs(l0)), (l0, l1)
    assert dg < 2e-3 * sc


@pytest.mark.parametrize("B,Lh,vocab", [(5, 30, 4300), (3, 12, 100)])
def test_fused_loss_is_torchs_loss_on_the_same_logits(tmp_path, B, Lh, vocab):
    """Train mode, fixed dropout seed, the full decoder length on both calls (so both draw the same masks): the fp32 logits of
    forward_loss(want_logits=True) under float64 F.cross_entropy(label_smoothing=eps) against the fused loss of want_logits=False (and the
    materialised one that came with the logits).  Bound: the operator's loss bound + the 1e-5 relative that
    test_chains_equal_the_launch_per_operation_forward grants fused against unfused logits."""
    eps = 0.1
    cfg = _head_cfg(vocab)
    m = _model(cfg, tmp_path, 3 + B, label_smoothing=eps)
    m.trim_padding = False
    px, lab = synthetic_batch(cfg, B, Lh, seed=5 + B, min_chars=1, max_chars=Lh - 2)
    pxt, ids = torch.from_numpy(px).cuda(), torch.from_numpy(lab).cuda()
    m.train()
    loss_m, logits = m.forward_loss(pxt, ids, want_logits=True, seed=13)
    loss_m = float(loss_m)
    loss_f = float(m.forward_loss(pxt, ids, want_logits=False, seed=13)[0])
    tgt = ids[:, 1:].reshape(-1)
    want = _ce64(logits.reshape(-1, vocab), tgt, eps, cfg.pad_id)
    plain = _ce64(logits.reshape(-1, vocab), tgt, 0.0, cfg.pad_id)
    tol = CE_LS_LOSS_BOUND + 1e-5 * abs(want)
    print(f"B={B} L={Lh} V={vocab}: fused {loss_f:.7f}, materialised {loss_m:.7f}, float64 {want:.7f} (plain {plain:.7f}); bound {tol:.3g}")
    assert abs(loss_f - want) <= tol and abs(loss_m - want) <= tol


def test_eval_mode_ignores_eps(tmp_path):
    """(7, 23, 777), m.eval(): the loss with label_smoothing 0.3 equals the loss with 0 within 2e-6 relative (float-atomic order), on the
    fused and on the materialised path, and all of them are the float64 PLAIN cross-entropy of the returned logits (the bound of the test
    above): val_loss stays the quantity the reference logs.  The tied embedding / head weight is scaled by 16 first: at the recipe's
    initialisation the logits are so flat that the smoothed and the plain loss of a batch lie closer than the bound, and the test could
    not tell them apart (asserted: they differ by more than 100 bounds here)."""
    B, Lh, vocab = 7, 23, 777
    cfg = _head_cfg(vocab)
    m = _model(cfg, tmp_path, 3 + B)
    m.state_dict_views()["decoder.roberta.embeddings.word_embeddings.weight"].mul_(16.0)      # before the first bind, which casts the weights
    px, lab = synthetic_batch(cfg, B, Lh, seed=5 + B, min_chars=1, max_chars=Lh - 2)
    pxt, ids = torch.from_numpy(px).cuda(), torch.from_numpy(lab).cuda()
    m.eval()
    got = {}
    for eps in (0.3, 0.0):
        m.label_smoothing = eps
        assert m.label_smoothing == eps
        lf = float(m.forward_loss(pxt, ids, want_logits=False)[0])
        lm, logits = m.forward_loss(pxt, ids, want_logits=True)
        got[eps] = (lf, float(lm), logits.clone())
    assert torch.equal(got[0.3][2], got[0.0][2])
    tgt = ids[:, 1:].reshape(-1)
    want = _ce64(got[0.0][2].reshape(-1, vocab), tgt, 0.0, cfg.pad_id)
    smoothed = _ce64(got[0.0][2].reshape(-1, vocab), tgt, 0.3, cfg.pad_id)
    tol = CE_LS_LOSS_BOUND + 1e-5 * abs(want)
    print(f"eval: fused {got[0.3][0]:.7f} / {got[0.0][0]:.7f}, materialised {got[0.3][1]:.7f} / {got[0.0][1]:.7f}, float64 plain {want:.7f} (smoothed {smoothed:.7f})")
    assert abs(smoothed - want) > 100 * tol
    for i in (0, 1):
        assert abs(got[0.3][i] - got[0.0][i]) < 2e-6 * max(1.0, abs(got[0.0][i]))
        assert abs(got[0.3][i] - want) <= tol and abs(got[0.0][i] - want) <= tol


# ================================================================================================ 5. the whole step
@pytest.mark.parametrize("fused", [False, True], ids=["materialised", "one-launch-head"])
def test_whole_step_against_the_oracle_with_torchs_smoothed_loss(tmp_path, fused):
    """test_parity_gpu.py::_replay_case with eps 0.1, dropout on: the oracle's network (O.forward with the step's own masks) gives the
    logits, the test applies F.cross_entropy(ignore_index=pad, label_smoothing=0.1) and calls backward.  tiny_config takes head GEMM +
    ce_kernel, the 256 / 4 / 768 decoder the one-launch head.  That function's metric and tolerances: per tensor max|have - want| /
    max|want| <= 0.05, loss within 5e-3, key.bias skipped.  The guard, from the oracle alone: the eps = 0 gradient of
    decoder.lm_head.bias misses the eps = 0.1 one by more than that tolerance, so an engine that ignored eps could not pass."""
    eps, grad_tol, B, Lh, seed, model_seed = 0.1, 0.05, 3, 24, 12345, 42
    cfg = dataclasses.replace(tiny_config(), dec_hidden=256, dec_heads=4, dec_ffn=768) if fused else tiny_config()
    m = _model(cfg, tmp_path, model_seed, label_smoothing=eps)
    m.trim_padding = False                      # the masks below are drawn for the full decoder length
    px, lab = synthetic_batch(cfg, B, Lh, seed=3, min_chars=3, max_chars=Lh - 1)
    m.train()
    m.zero_grad()
    loss, _ = m.forward_loss(torch.from_numpy(px), torch.from_numpy(lab), want_logits=False, seed=seed)
    m.backward()
    torch.cuda.synchronize()
    masks = step_masks(cfg, seed, B, Lh - 1)
    assert len(masks) == 1 + 3 * cfg.enc_layers + 1 + 5 * cfg.dec_layers
    leaves = O.leaf_state_dict(P.state_dict_from_flat(cfg, P.recipe_flat(cfg, model_seed)))
    labt = torch.from_numpy(lab)
    logits, plain = O.forward(cfg, leaves, torch.from_numpy(px), labt, masks=masks)
    want_loss = F.cross_entropy(logits.reshape(-1, logits.shape[-1]), labt[:, 1:].reshape(-1), ignore_index=cfg.pad_id, label_smoothing=eps)
    bias = leaves["decoder.lm_head.bias"]
    g_plain = torch.autograd.grad(plain, bias, retain_graph=True)[0]
    want_loss.backward()
    miss = float((g_plain - bias.grad).abs().max() / (bias.grad.abs().max() + 1e-9))
    print(f"oracle: loss {float(want_loss):.5f} smoothed / {float(plain):.5f} plain; lm_head.bias gradient without eps misses by {miss:.3g}")
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


# ================================================================================================ 6. range and round trip
def test_range_and_checkpoint_round_trip(tmp_path, lib):
    from kzv.trainer import load_checkpoint, save_checkpoint
    cfg = micro_config()
    d = build_decoder_dir(str(tmp_path / "dec"), cfg)
    golden = os.path.join(HERE, "golden", "micro_lightning.ckpt")
    enc = torch.load(golden, map_location="cpu", weights_only=False)["hyper_parameters"]["encoder_config"]
    m = TrOCRModel(enc, d, init_seed=1, load_tokenizer=False)
    assert m.label_smoothing == 0.0 and lib.kzv_get_label_smoothing(m._h) == 0.0 and m.hparams.label_smoothing == 0.0
    assert lib.kzv_set_label_smoothing(m._h, 1.0) == -1          # KZV_E_ARG
    assert lib.kzv_set_label_smoothing(m._h, -0.1) == -1
    assert lib.kzv_set_label_smoothing(m._h, float("nan")) == -1
    assert lib.kzv_get_label_smoothing(m._h) == 0.0
    for bad in (1.0, -0.1):
        with pytest.raises(ValueError):
            TrOCRModel(enc, d, init_seed=1, load_tokenizer=False, label_smoothing=bad)
        with pytest.raises(ValueError):
            m.label_smoothing = bad
    # the operator refuses it too
    z = torch.zeros(1, 8, device=DEV); lab = torch.full((1, 2), 2, dtype=torch.int64, device=DEV); one = torch.ones(1, device=DEV)
    assert lib.kzv_ce_fwd_bwd_ls(z.data_ptr(), 8, lab.data_ptr(), 2, 1, 1, 8, PAD, one.data_ptr(), one.data_ptr(), None, 1.0, _st()) == -1
    m.label_smoothing = 0.1
    assert m.label_smoothing == 0.1 and abs(lib.kzv_get_label_smoothing(m._h) - 0.1) < 1e-8
    path = tmp_path / "smoothed.ckpt"
    save_checkpoint(m, None, str(path), 0, 1)
    assert torch.load(path, map_location="cpu", weights_only=False)["hyper_parameters"]["label_smoothing"] == 0.1
    m2 = TrOCRModel(enc, d, init_seed=2, load_tokenizer=False)
    load_checkpoint(m2, None, str(path))
    assert m2.label_smoothing == 0.1 and abs(lib.kzv_get_label_smoothing(m2._h) - 0.1) < 1e-8
    assert torch.equal(m2.flat_params, m.flat_params)
    # a reference checkpoint has no such key: the plain loss
    load_checkpoint(m2, None, golden)
    assert m2.label_smoothing == 0.0 and lib.kzv_get_label_smoothing(m2._h) == 0.0
