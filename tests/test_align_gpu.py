"""Per-character confidence and position at the model level: kzv_cross_attention / kzv_score_tokens and TrOCRModel.align /
recognize against the oracle (oracle/trocr_oracle.py, untouched: its ``_drop`` is wrapped to record the softmax output
[B, heads, T, Sk] of every decoder cross-attention; the mean over heads is what HF returns as cross_attentions[i].mean(1)).

The map bound is not fixed in advance: ``err_ref`` is the same oracle run with a bf16 state dict and bf16 pixels, measured against
the fp32 oracle on live rows; the engine (bf16 operands, fp32 accumulation and softmax) must stay within 2 x err_ref per layer.
The margin of 2 allows for the engine's rounding points not being the all-bf16 oracle's.  Peaks must equal the oracle's arg-max
wherever the oracle's two largest weights are further apart than twice the engine's measured error (at least 60 % of the live
rows), centroids stay within sum_k |dP| x the grid extent.

Measured on an MI355X (engine error / err_ref): see DESIGN.md section 7, "Per-character confidence and position"."""
import ctypes as C
import dataclasses

import numpy as np
import pytest
import torch

from kzv import _lib as L
from kzv import params as P
from kzv.config import tiny_config
from kzv.data import build_decoder_dir, synthetic_batch
from kzv.model import TrOCRModel
from oracle import trocr_oracle as O

from _trained import load

pytestmark = pytest.mark.gpu
LOGIT_TOL = 3e-2          # tests/test_trained_gpu.py


@pytest.fixture(autouse=True)
def _default_modes_afterwards():
    yield
    L.load().kzv_set_dec_chain(-1)
    L.load().kzv_set_head_ce(-1)


def oracle_maps(cfg, sd_np, px, lab, dtype=torch.float32):
    """-> ([B, T, Sk] fp32 head-mean cross-attention map per decoder layer, logits [B, T, V] fp32) of the oracle in `dtype`."""
    seen = []
    orig = O._drop

    def spy(x, masks, name):
        if isinstance(name, str) and name.endswith("_ca"):
            seen.append(x.detach().float())
        return orig(x, masks, name)

    sd = O.leaf_state_dict(sd_np, dtype=dtype, requires_grad=False)
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(O, "_drop", spy)
        with torch.no_grad():
            logits, _ = O.forward(cfg, sd, torch.as_tensor(px).to(dtype), torch.as_tensor(lab))
    assert len(seen) == cfg.dec_layers
    return [p.mean(1) for p in seen], logits.float()


def live_rows(lab, pad_id):
    lab = torch.as_tensor(lab)
    return (lab[:, :-1] != pad_id) & (lab[:, 1:] != pad_id)


def check_maps(tag, cfg, m, px, lab, ref32, ref16, width=None):
    """The assertions of the module docstring for every layer of one batch; returns the measured figures."""
    live = live_rows(lab, cfg.pad_id)
    assert int(live.sum()) > 0
    grid_w = (width or cfg.image_w) // cfg.patch_w
    n_rows = cfg.image_h // cfg.patch_h
    k = torch.arange(ref32[0].shape[-1])
    row, col = (k // grid_w).float(), (k % grid_w).float()
    figures = []
    for layer in range(cfg.dec_layers):
        out = m.align(torch.from_numpy(px), torch.from_numpy(lab), layer=layer, want_map=True)
        torch.cuda.synchronize()
        assert bool(out["live"].cpu().eq(live).all())
        got = out["map"].cpu()
        assert got.shape == ref32[layer].shape and bool(torch.isfinite(got).all())
        want = ref32[layer]
        err = float((got - want)[live].abs().max())
        err_ref = float((ref16[layer] - want)[live].abs().max())
        top2 = torch.topk(want, 2, dim=-1).values
        decided = ((top2[..., 0] - top2[..., 1]) > 2 * err) & live
        frac = float(decided.sum()) / float(live.sum())
        med_peak = float(want.max(-1).values[live].median())
        row_sum = float((out["row_sum"].cpu()[live] - 1).abs().max())
        print(f"{tag} layer {layer}: engine err {err:.4g}, err_ref {err_ref:.4g}, decided {frac:.3f}, median peak {med_peak:.3f}, |row sum - 1| {row_sum:.2g}")
        figures.append((err, err_ref, frac))
        assert err <= 2 * err_ref, (tag, layer, err, err_ref)
        assert row_sum < 1e-3
        assert frac >= 0.60, (tag, layer, frac)
        assert bool((out["peak_patch"].cpu().long()[decided] == want.argmax(-1)[decided]).all())
        assert bool(torch.allclose(out["peak_weight"].cpu()[live], got.max(-1).values[live], rtol=0, atol=1e-6))
        # centroids: |sum_k dP row_k| <= sum_k |dP| * rows (in pixels: * patch_h), likewise the columns
        l1 = (got - want).abs().sum(-1)
        cen = out["centroid"].cpu()
        want_y, want_x = ((want * row).sum(-1) + 0.5) * cfg.patch_h, ((want * col).sum(-1) + 0.5) * cfg.patch_w
        assert bool(((cen[..., 0] - want_y).abs() <= l1 * n_rows * cfg.patch_h)[live].all())
        assert bool(((cen[..., 1] - want_x).abs() <= l1 * grid_w * cfg.patch_w)[live].all())
        assert bool(((cen[..., 0] >= 0) & (cen[..., 0] <= cfg.image_h) & (cen[..., 1] >= 0) & (cen[..., 1] <= grid_w * cfg.patch_w))[live].all())
    return figures


# ------------------------------------------------------------------------------------------------ the fitted tiny model
@pytest.fixture(scope="module")
def trained(tmp_path_factory):
    g, cfg, sd, data = load()
    d = build_decoder_dir(str(tmp_path_factory.mktemp("dec")), cfg)
    m = TrOCRModel(cfg.encoder_config_dict(), d, load_tokenizer=True)
    m.load_state_dict(sd, strict=True)
    m.eval()
    refs = {tag: (oracle_maps(cfg, sd, px, lab), oracle_maps(cfg, sd, px, lab, torch.bfloat16)) for tag, (px, lab) in data.items()}
    return g, cfg, sd, data, m, refs


def test_cross_attention_maps_of_the_fitted_model_against_the_oracle(trained):
    g, cfg, sd, data, m, refs = trained
    for tag, (px, lab) in data.items():
        (ref32, _), (ref16, _) = refs[tag]
        check_maps(tag, cfg, m, px, lab, ref32, ref16)


def test_several_layers_average_their_maps(trained):
    g, cfg, sd, data, m, refs = trained
    px, lab = data["fit"]
    pxt, labt = torch.from_numpy(px), torch.from_numpy(lab)
    one = [m.align(pxt, labt, layer=i, want_map=True) for i in range(cfg.dec_layers)]
    both = m.align(pxt, labt, layer=(0, -1), want_map=True)
    mean = (one[0]["map"] + one[-1]["map"]) / 2
    live = both["live"]
    assert bool(torch.allclose(both["map"], mean, rtol=0, atol=1e-7))
    assert bool(torch.allclose(both["peak_weight"][live], mean.max(-1).values[live], rtol=0, atol=1e-7))
    assert bool(torch.equal(both["logprob"], one[0]["logprob"]))
    no_map = m.align(pxt, labt, layer=-1)
    assert "map" not in no_map and bool(torch.equal(no_map["peak_patch"], one[-1]["peak_patch"])) and bool(torch.equal(no_map["centroid"], one[-1]["centroid"]))
    with pytest.raises(ValueError):
        m.align(pxt, labt, layer=cfg.dec_layers)


def test_token_scores_of_the_fitted_model(trained):
    g, cfg, sd, data, m, refs = trained
    for tag, (px, lab) in data.items():
        pxt, labt = torch.from_numpy(px), torch.from_numpy(lab)
        logits = m(pxt, labt)["logits"]
        out = m.align(pxt, labt)
        torch.cuda.synchronize()
        live = out["live"]
        tgt = labt[:, 1:].to(logits.device)
        ls = torch.log_softmax(logits.double(), -1)
        want = torch.gather(ls, 2, tgt[:, :, None]).squeeze(-1)
        err = float((out["logprob"].double() - want)[live].abs().max())
        err_top = float((out["top1_logprob"].double() - ls.max(-1).values)[live].abs().max())
        # the fixture's reference logits: log-softmax moves by at most the logit error twice (the target's and the log-sum-exp's)
        ref_logits = torch.from_numpy(g[f"{tag}/logits"]).double()
        ref_lp = torch.gather(torch.log_softmax(ref_logits, -1), 2, labt[:, 1:, None]).squeeze(-1)
        tol = max(LOGIT_TOL, 4e-3 * float(ref_logits.abs().max()))
        err_ref = float((out["logprob"].cpu().double() - ref_lp)[live.cpu()].abs().max())
        print(f"{tag}: |logprob - log_softmax(engine logits)| {err:.3g}, top1 {err_top:.3g}; against the reference's logits {err_ref:.3g} (bound {2 * tol:.3g})")
        assert err <= 1e-4 and err_top <= 1e-4            # the same GEMM, an fp32 row reduction over 157 entries
        assert bool(torch.equal(out["top1"][live], logits.argmax(-1)[live]))
        assert err_ref <= 2 * tol
        # padded positions: target pad -> 0
        assert bool((out["logprob"][tgt == cfg.pad_id] == 0).all())


def test_recognize_on_the_fitted_batch(trained):
    g, cfg, sd, data, m, refs = trained
    px = torch.from_numpy(data["fit"][0])
    rec = m.recognize(px)
    texts = m.decode_predictions(px)
    assert [r["text"] for r in rec] == texts
    for r in rec:
        # a one-character vocabulary: as many tokens as characters
        assert len(r["tokens"]) == len(r["text"]) == len(r["token_strings"]) == len(r["logprobs"]) == len(r["centroids"]) == len(r["peak_patches"])
        assert 0.0 < r["confidence"] <= 1.0
        assert all(lp <= 0.0 for lp in r["logprobs"])
        assert all(0 <= y <= cfg.image_h and 0 <= x <= cfg.image_w for y, x in r["centroids"])
        assert all(0 <= p < cfg.num_patches for p in r["peak_patches"])
    print("recognize: " + ", ".join(f"{r['text']!r} {r['confidence']:.3f}" for r in rec[:4]))


def test_state_rules(trained):
    g, cfg, sd, data, m, refs = trained
    lib = L.load()
    px, lab = data["fit"]
    pxt, labt = torch.from_numpy(px), torch.from_numpy(lab)
    B, Lh = lab.shape
    buf = torch.empty(B * Lh * 4, dtype=torch.float32, device="cuda")
    ibuf = torch.empty(B * Lh, dtype=torch.int64, device="cuda")

    def both_refuse(why):
        st = L.stream_handle()
        assert lib.kzv_cross_attention(m._h, -1, None, 0, buf.data_ptr(), ibuf.data_ptr(), st) == -3, why
        assert b"cross_attention" in lib.kzv_last_error()
        assert lib.kzv_score_tokens(m._h, buf.data_ptr(), ibuf.data_ptr(), None, st) == -3, why
        with pytest.raises(L.KzvError):
            m.align_last()

    m.align(pxt, labt)
    step_logits = torch.empty(B, cfg.vocab, dtype=torch.float32, device="cuda")
    L.check(lib.kzv_decode_logits(m._h, m._keep[1].data_ptr(), 0, step_logits.data_ptr(), L.stream_handle()), "decode_logits")
    both_refuse("after kzv_decode_logits")
    m.align(pxt, labt)
    m.generate(pxt, max_length=Lh, num_beams=1)
    both_refuse("after generate")
    m.align(pxt, labt)
    L.check(lib.kzv_set_active_length(m._h, 1), "set_active_length")
    both_refuse("after a change of the active length")
    # a training-mode forward: the read-backs in between change neither the loss nor the gradients
    m.train()
    try:
        m.zero_grad()
        loss_a, _ = m.forward_loss(pxt, labt, seed=5)
        m.backward()
        torch.cuda.synchronize()
        la, ga = float(loss_a), m.flat_grads.clone()
        loss_b, _ = m.forward_loss(pxt, labt, seed=5)
        lb = float(loss_b)
        out = m.align_last(layer=(0, 1), want_map=True)
        assert bool(torch.isfinite(out["map"]).all()) and bool(torch.isfinite(out["logprob"]).all())
        m.backward()
        torch.cuda.synchronize()
        gb = m.flat_grads.clone()
        assert float(m._loss) == lb                                      # the read-backs leave the loss alone ...
    finally:
        m.eval()
    assert abs(la - lb) <= 2e-6 * max(1.0, abs(la))                      # ... and it is the first forward's (a sum of float atomics)
    sc = float(ga.abs().max())
    assert sc > 0 and float((ga - gb).abs().max()) <= 1e-5 * sc          # float-atomic order at most


# ------------------------------------------------------------------------------------------------ the reference decoder's geometry
@pytest.fixture(scope="module")
def wide(tmp_path_factory):
    """Hidden 256, 4 heads, FFN 768 (the chain kernels write cq), 2 decoder layers, a 1-layer 128-wide encoder on 64 x 640
    (160 keys), B = 3, random init; the test's own copy of every crossattention.self.query.weight is scaled up (x 2 per round)
    until the oracle's median peak weight on live rows exceeds 0.2."""
    cfg = dataclasses.replace(tiny_config(), image_h=64, image_w=640, enc_hidden=128, enc_layers=1, enc_heads=2, enc_ffn=256,
                              dec_hidden=256, dec_heads=4, dec_ffn=768, dec_layers=2, vocab=4300, max_pos=128)
    sd = {k: np.array(v, copy=True) for k, v in P.state_dict_from_flat(cfg, P.recipe_flat(cfg, 11)).items()}
    batches = {"trimmed": synthetic_batch(cfg, 3, 40, seed=21, min_chars=3, max_chars=17),
               "untrimmed": synthetic_batch(cfg, 3, 20, seed=22, min_chars=19, max_chars=19)}
    px, lab = batches["trimmed"]
    live = live_rows(lab, cfg.pad_id)
    keys = [f"decoder.roberta.encoder.layer.{i}.crossattention.self.query.weight" for i in range(cfg.dec_layers)]
    factor = 1.0
    for _ in range(16):
        maps, _ = oracle_maps(cfg, sd, px, lab)
        med = min(float(p.max(-1).values[live].median()) for p in maps)
        if med > 0.2:
            break
        for k in keys:
            sd[k] *= 2.0
        factor *= 2.0
    print(f"cross-attention query weights x {factor:g}: median oracle peak weight {med:.3f}")
    assert med > 0.2
    d = build_decoder_dir(str(tmp_path_factory.mktemp("decw")), cfg)
    m = TrOCRModel(cfg.encoder_config_dict(), d, load_tokenizer=False)
    m.load_state_dict(sd, strict=True)
    m.eval()
    refs = {tag: (oracle_maps(cfg, sd, px, lab), oracle_maps(cfg, sd, px, lab, torch.bfloat16)) for tag, (px, lab) in batches.items()}
    return cfg, sd, batches, m, refs


@pytest.mark.parametrize("tag", ["trimmed", "untrimmed"])
def test_cross_attention_maps_at_the_reference_decoder_geometry(wide, tag):
    cfg, sd, batches, m, refs = wide
    px, lab = batches[tag]
    (ref32, _), (ref16, _) = refs[tag]
    lib = L.load()
    maps = {}
    for chain in (0, 2):
        L.check(lib.kzv_set_dec_chain(chain), "set_dec_chain")
        check_maps(f"{tag} chain {chain}", cfg, m, px, lab, ref32, ref16)
        n_live = int((torch.from_numpy(lab) != cfg.pad_id).sum(dim=1).max())
        assert m.last_active_length == (min(lab.shape[1] - 1, n_live))
        maps[chain] = [m.align(torch.from_numpy(px), torch.from_numpy(lab), layer=i, want_map=True)["map"] for i in range(cfg.dec_layers)]
    assert (m.last_active_length < lab.shape[1] - 1) == (tag == "trimmed")
    for a, b in zip(maps[0], maps[2]):
        assert float((a - b).abs().max()) <= 1e-6


def test_token_scores_after_the_one_launch_head(wide):
    """align's forward asks for no logits: at this geometry it takes the one-launch LM head + cross-entropy, which never writes
    them; kzv_score_tokens re-runs the vocabulary GEMM from the saved head input.  Against log_softmax of the logits that
    model(px, labels) returns (head GEMM path), 4,300 entries per row."""
    cfg, sd, batches, m, refs = wide
    lib = L.load()
    for tag, (px, lab) in batches.items():
        pxt, labt = torch.from_numpy(px), torch.from_numpy(lab)
        logits = m(pxt, labt)["logits"]
        L.check(lib.kzv_set_head_ce(1), "set_head_ce")
        out = m.align(pxt, labt)
        torch.cuda.synchronize()
        live = out["live"]
        ls = torch.log_softmax(logits.double(), -1)
        want = torch.gather(ls, 2, labt[:, 1:, None].to(logits.device)).squeeze(-1)
        err = float((out["logprob"].double() - want)[live].abs().max())
        err_top = float((out["top1_logprob"].double() - ls.max(-1).values)[live].abs().max())
        print(f"{tag}: |logprob - log_softmax(returned logits)| {err:.3g}, top1 {err_top:.3g}")
        assert err <= 1e-4 and err_top <= 1e-4
        assert bool(torch.equal(out["top1"][live], logits.argmax(-1)[live]))
        # ... and against the fp32 oracle's logits, at the tolerance of flat logits doubled
        ref_lp = torch.gather(torch.log_softmax(refs[tag][0][1].double(), -1), 2, labt[:, 1:, None]).squeeze(-1)
        assert float((out["logprob"].cpu().double() - ref_lp)[live.cpu()].abs().max()) <= 2 * LOGIT_TOL
