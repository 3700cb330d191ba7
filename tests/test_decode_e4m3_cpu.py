"""Generation from e4m3 decoder weights (include/kzv.h: kzv_set_decode_weights), the parts that need no GPU:

  * the ABI's states: the setter takes 0 / 1 and nothing else, the getter round-trips, kzv_decode_weights_impl is a state error
    before kzv_model_bind (like kzv_decode_step_impl) and launches nothing;
  * the recipe, kzv/quant.py: row_pow2_e4m3 equals the oracle's restatement of the format, quant_e4m3(w / s), bit for bit -- random
    rows over many decades, an all-zero row, rows whose amax is exactly 448 * 2^k, values on rounding ties, values in the e4m3
    subnormal range; q * s survives a bf16 round trip unchanged (what makes the GPU test exact); amax / s lies in (224, 448];
  * what the recipe costs the reference-fitted fixture (tests/golden/tiny_trained.npz) under the oracle: greedy_stepwise decodes the
    same tokens from the dequantised weights as from the original ones, on the crops it was fitted on and on unseen ones.  Every
    decoder Linear of the quantised set is replaced, whatever the engine would do with this 64-wide decoder."""
import ctypes as C
import os

import numpy as np
import torch

from _e4m3 import special_rows
from kzv import _lib as L
from kzv import quant as Q
from kzv.config import tiny_config
from oracle import trocr_oracle as O


def _handle(lib):
    cfg = tiny_config()
    c = L.kzv_config(image_h=cfg.image_h, image_w=cfg.image_w, patch_h=cfg.patch_h, patch_w=cfg.patch_w, channels=cfg.channels,
                     enc_hidden=cfg.enc_hidden, enc_layers=cfg.enc_layers, enc_heads=cfg.enc_heads, enc_ffn=cfg.enc_ffn,
                     dec_hidden=cfg.dec_hidden, dec_layers=cfg.dec_layers, dec_heads=cfg.dec_heads, dec_ffn=cfg.dec_ffn,
                     vocab=cfg.vocab, max_pos=cfg.max_pos, type_vocab=cfg.type_vocab, pad_id=cfg.pad_id, ln_eps=1e-12)
    h = C.c_void_p()
    L.check(lib.kzv_model_create(C.byref(c), C.byref(h)), "create")
    return h


def test_decode_weights_abi_states():
    if not os.path.exists(L.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    lib = L.load()
    h = _handle(lib)
    try:
        assert lib.kzv_get_decode_weights(h) == 0                       # bf16 is the default
        assert lib.kzv_set_decode_weights(h, 2) < 0
        assert b"set_decode_weights" in lib.kzv_last_error() and b"e4m3" in lib.kzv_last_error()
        assert lib.kzv_set_decode_weights(h, -1) < 0
        assert lib.kzv_get_decode_weights(h) == 0                       # a rejected format changes nothing
        assert lib.kzv_set_decode_weights(h, 1) == 0 and lib.kzv_get_decode_weights(h) == 1
        assert lib.kzv_decode_weights_impl(h) < 0                       # not bound: an error, not an answer
        assert b"decode_weights_impl" in lib.kzv_last_error()
        assert lib.kzv_decode_weights_impl(None) < 0
        assert lib.kzv_set_decode_weights(None, 1) < 0 and lib.kzv_get_decode_weights(None) < 0
        assert lib.kzv_set_decode_weights(h, 0) == 0 and lib.kzv_get_decode_weights(h) == 0
    finally:
        lib.kzv_model_destroy(h)


def test_recipe_equals_the_oracle_restatement_bit_for_bit():
    gen = torch.Generator().manual_seed(0)
    K = 256
    rand = torch.randn(400, K, generator=gen) * 10 ** torch.empty(400, 1).uniform_(-6, 4, generator=gen)
    w = torch.cat([special_rows(K, gen), rand]).to(torch.bfloat16).to(torch.float32)
    q, s = Q.row_pow2_e4m3(w)
    assert q.dtype == torch.float8_e4m3fn and s.dtype == torch.float32 and tuple(s.shape) == (w.shape[0],)
    qf = q.to(torch.float32)
    assert torch.equal(qf, O.quant_e4m3(w / s[:, None]))                 # the format restated, against torch's own cast
    assert float(s[0]) == 1.0 and not qf[0].any()                        # the all-zero row
    m, e = torch.frexp(s)
    assert torch.equal(m, torch.full_like(m, 0.5))                       # every scale is a power of two
    amax = w.abs().amax(-1)
    ratio = (amax / s)[amax > 0]
    assert bool((ratio > 224).all()) and bool((ratio <= 448).all())
    assert [float(x) for x in (amax / s)[1:5]] == [448.0] * 4 and 224 < float((amax / s)[5]) < 232
    deq = Q.dequantise(q, s)
    assert torch.equal(deq.to(torch.bfloat16).to(torch.float32), deq)    # q * s IS a bf16 number
    rel = ((deq - w).abs().amax(-1) / amax.clamp_min(1e-30))[amax > 0]
    # half an e4m3 step: 16 where amax / s is in [256, 448], 8 where it is in (224, 256) -- at most 1 / 16 of amax either way
    assert float(rel.max()) <= 1 / 16
    # an fp32 weight is rounded to bf16 first, as the engine's weight copies are
    w32 = torch.randn(16, K, generator=gen)
    q32, s32 = Q.row_pow2_e4m3(w32)
    q16, s16 = Q.row_pow2_e4m3(w32.to(torch.bfloat16))
    assert torch.equal(q32.view(torch.uint8), q16.view(torch.uint8)) and torch.equal(s32, s16)


def test_quantised_set_by_hf_name():
    names = {f"decoder.roberta.encoder.layer.3.{n}.weight": True for n in Q.LAYER_LINEARS}
    names.update({"decoder.lm_head.dense.weight": True, "decoder.lm_head.dense.bias": False,
                  "decoder.roberta.encoder.layer.3.crossattention.self.key.weight": False,
                  "decoder.roberta.encoder.layer.3.crossattention.self.value.weight": False,
                  "decoder.roberta.encoder.layer.3.attention.output.LayerNorm.weight": False,
                  "decoder.roberta.encoder.layer.3.attention.self.query.bias": False,
                  "decoder.roberta.embeddings.word_embeddings.weight": False, "decoder.lm_head.decoder.weight": False,
                  "encoder.layers.3.attention.attention.query.weight": False, "encoder_decoder_proj.weight": False})
    for n, want in names.items():
        assert Q.is_quantised(n) == want, n
    assert len(Q.LAYER_LINEARS) == 8


def test_recipe_keeps_the_fitted_fixtures_greedy_decodes():
    from _trained import load
    g, cfg, sd, data = load()
    tsd = O.leaf_state_dict(sd, requires_grad=False)
    dq = Q.dequantised_decoder_weights(tsd)
    changed = [k for k in tsd if not torch.equal(tsd[k], dq[k])]
    assert len(changed) == 8 * cfg.dec_layers + 1 and all(Q.is_quantised(k) for k in changed)
    worst_w = max(float(((dq[k] - tsd[k]).abs().amax(-1) / tsd[k].abs().amax(-1)).max()) for k in changed)
    print(f"worst relative weight error {worst_w:.3%}")
    assert worst_w <= 1 / 16                                             # half an e4m3 step over amax, see above
    for tag, (px, lab) in data.items():
        ids, gaps = O.greedy_stepwise(cfg, tsd, px, int(g["label_len"]))
        ids_q, _ = O.greedy_stepwise(cfg, dq, px, int(g["label_len"]))
        a, _ = O.forward(cfg, tsd, torch.from_numpy(px), torch.from_numpy(lab))
        b, _ = O.forward(cfg, dq, torch.from_numpy(px), torch.from_numpy(lab))
        print(f"{tag}: largest teacher-forced logit shift {float((a - b).abs().max()):.2f}, logit span {float(a.max() - a.min()):.1f}, "
              f"smallest top-2 gap of the original decode {float(gaps[np.isfinite(gaps)].min()):.2f}")
        assert np.array_equal(ids, g[f"{tag}/greedy_ids"])
        assert np.array_equal(ids_q, ids), tag
