"""A model whose decoder attention is PEAKED, built from the oracle alone (oracle/trocr_oracle.py, untouched: its ``_drop`` is wrapped
to record the softmax output of every decoder self- and cross-attention, as tests/test_align_gpu.py does for the cross-attention).

On recipe weights, N(0, 0.02), both attentions of the decoder are uniform (largest cross-attention weight 0.007 over 160 keys) and the
logits do not notice the softmax scale (halving it moves them by 8e-5).  ``peaked`` therefore

  1. starts from the recipe state dict of ``seed``;
  2. multiplies attention.self.value and crossattention.self.value (weight and bias) of every decoder layer by 8, so that the attention
     output is a sizeable part of the residual stream;
  3. doubles attention.self.query (weight and bias, all layers together) until the fp32 oracle's self-attention is peaked, and
     separately crossattention.self.query until its cross-attention is, at most 16 rounds each.  Peaked: per layer the median, over
     live rows and heads, of the largest probability of the row; the smallest layer value above 0.3.  Self-attention counts only rows
     with at least 8 keys;
  4. rounds every tensor and the pixels to bf16 and back, so that the engine and every oracle run read the same numbers (done before
     step 2: all factors are powers of two and commute with the rounding).

``conditions`` measures the result on a batch and asserts the two conditions the GPU tests rest on:
  * peakedness: both medians above 0.3;
  * discrimination: min(sens_self, sens_cross) >= 6 * err_ref, where err_ref = max |logits(oracle, all bf16) - logits(oracle, fp64)|
    and sens_* = the largest change of the fp64 logits when the self (cross) query weight and bias of all layers are halved, i.e.
    when that attention's softmax scale is wrong by a factor 2.  The GPU tests allow 2 x err_ref: an error of that kind is three
    times their bound.

A batch is (px [images, C, H, W], lab [rows, Lh]) with rows a multiple of images (rows i*k .. i*k+k-1 read image i, as the beams of a
search do); lab[:, 0] is BOS and padding only trails.  The decoder input is lab[:, :-1]; a row of logits is live where its input token
is not padding, and has t + 1 keys at column t."""
import dataclasses

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from kzv import params as P
from kzv.config import tiny_config
from kzv.data import synthetic_batch
from oracle import trocr_oracle as O

VALUE_GAIN = 8.0
PEAK = 0.3
MIN_KEYS = 8
ROUNDS = 16
RATIO = 6.0
LAYER = "decoder.roberta.encoder.layer.{}.{}.self.{}"


def geometry(image_h=64, image_w=640, dec_layers=3):
    """Decoder 256 / 4 heads / FFN 768, vocabulary 4300, 128 positions; a 1-layer 128-wide encoder with 2 heads; dropout off."""
    return dataclasses.replace(tiny_config(), image_h=image_h, image_w=image_w, enc_hidden=128, enc_layers=1, enc_heads=2, enc_ffn=256,
                               dec_hidden=256, dec_heads=4, dec_ffn=768, dec_layers=dec_layers, vocab=4300, max_pos=128,
                               enc_hidden_dropout=0.0, enc_attn_dropout=0.0, dec_hidden_dropout=0.0, dec_attn_dropout=0.0)


def batch(cfg, images, rows_per_image, Lh, seed):
    """tests/test_decode_fused_gpu.py::_lockstep's batch: one crop per image, ragged row ends, BOS in column 0."""
    px, lab = synthetic_batch(cfg, images * rows_per_image, Lh, seed=seed, min_chars=2, max_chars=Lh - 2)
    lab[:, 0] = cfg.bos_id
    return px[::rows_per_image].copy(), lab


def bf16_exact(a):
    t = torch.as_tensor(np.asarray(a, dtype=np.float32))
    return t.to(torch.bfloat16).to(torch.float32).numpy()


def _keys(cfg, block, what):
    return [LAYER.format(i, block, f"{what}.{p}") for i in range(cfg.dec_layers) for p in ("weight", "bias")]


def scaled(cfg, sd, block, what, factor):
    """A copy of ``sd`` with ``block``.self.``what`` (weight and bias) of every decoder layer multiplied by ``factor``."""
    out = dict(sd)
    for k in _keys(cfg, block, what):
        out[k] = sd[k] * np.float32(factor)
    return out


def encode(cfg, sd_np, px, dtype):
    """-> (torch state dict in ``dtype``, the decoder's encoder input [images, Sk, dec_hidden] in ``dtype``)."""
    sd = O.leaf_state_dict(sd_np, dtype=dtype, requires_grad=False)
    with torch.no_grad():
        enc = O.encoder_forward(cfg, sd, torch.as_tensor(px).to(dtype))
        if cfg.has_proj:
            enc = F.linear(enc, sd["encoder_decoder_proj.weight"], sd["encoder_decoder_proj.bias"])
    return sd, enc


def decode(cfg, sd, ids, enc, probs=None):
    """Teacher-forced oracle logits [rows, T, V] of ``ids`` [rows, T]; ``enc`` [images, ...] is repeated to the rows.  ``probs``: a dict
    that receives {"sa": [per layer [rows, heads, T, T]], "ca": [per layer [rows, heads, T, Sk]]}, the softmax outputs."""
    ids = torch.as_tensor(ids)
    enc = enc.repeat_interleave(ids.shape[0] // enc.shape[0], dim=0)
    if probs is None:
        with torch.no_grad():
            return O.decoder_forward(cfg, sd, ids, enc)
    seen = {"sa": [], "ca": []}
    orig = O._drop

    def spy(x, masks, name):
        if isinstance(name, str) and name[-3:] in ("_sa", "_ca"):
            seen[name[-2:]].append(x.detach().float())
        return orig(x, masks, name)

    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(O, "_drop", spy)
        with torch.no_grad():
            out = O.decoder_forward(cfg, sd, ids, enc)
    assert len(seen["sa"]) == len(seen["ca"]) == cfg.dec_layers
    probs.update(seen)
    return out


def live_rows(cfg, ids):
    """(live [rows, T], live with at least MIN_KEYS keys [rows, T]) of decoder input ``ids``."""
    ids = torch.as_tensor(ids)
    live = ids != cfg.pad_id
    many = live & (torch.arange(ids.shape[1]) >= MIN_KEYS - 1)[None, :]
    return live, many


def peaks(cfg, sd, ids, enc):
    """(self, cross): the smallest over layers of the median, over live rows and heads, of the largest probability in the row."""
    live, many = live_rows(cfg, ids)
    assert int(many.sum()) > 0, "no live row with 8 keys"
    pr = {}
    decode(cfg, sd, ids, enc, pr)
    heads = cfg.dec_heads
    med = lambda p, rows: float(p.max(-1).values[rows[:, None, :].expand(-1, heads, -1)].median())
    return min(med(p, many) for p in pr["sa"]), min(med(p, live) for p in pr["ca"])


def sharpen(cfg, seed, px, lab):
    """Steps 1 - 4 of the module docstring -> (state dict of bf16-exact fp32 arrays, bf16-exact pixels, (self factor, cross factor))."""
    # Rounded first: every factor below is a power of two, which commutes with the rounding, so the rounds already judge the numbers
    # that are returned (judged before the rounding, a peak of 0.30 has come out as 0.29 after it).
    sd = {k: bf16_exact(v) for k, v in P.state_dict_from_flat(cfg, P.recipe_flat(cfg, seed)).items()}
    px = bf16_exact(px)
    for block in ("attention", "crossattention"):
        sd = scaled(cfg, sd, block, "value", VALUE_GAIN)
    ids = torch.as_tensor(lab)[:, :-1]
    enc = encode(cfg, sd, px, torch.float32)[1]                       # the encoder does not read what the rounds change
    factors = []
    for which, block in enumerate(("attention", "crossattention")):
        factor = 1.0
        for _ in range(ROUNDS):
            if peaks(cfg, O.leaf_state_dict(sd, dtype=torch.float32, requires_grad=False), ids, enc)[which] > PEAK:
                break
            sd = scaled(cfg, sd, block, "query", 2.0)
            factor *= 2.0
        factors.append(factor)
    sd = {k: bf16_exact(v) for k, v in sd.items()}                    # changes nothing unless a product left bf16's range
    return sd, px, tuple(factors)


def conditions(cfg, sd, px, lab, check=True):
    """The figures of the module docstring for state dict ``sd`` on one batch; with ``check`` both conditions are asserted."""
    ids = torch.as_tensor(lab)[:, :-1]
    live, many = live_rows(cfg, ids)
    sd32, enc32 = encode(cfg, sd, px, torch.float32)
    peak_self, peak_cross = peaks(cfg, sd32, ids, enc32)
    sd64, enc64 = encode(cfg, sd, px, torch.float64)
    ref = decode(cfg, sd64, ids, enc64)
    sd16, enc16 = encode(cfg, sd, px, torch.bfloat16)
    err_ref = float((decode(cfg, sd16, ids, enc16).double() - ref)[live].abs().max())
    sens = []
    for block in ("attention", "crossattention"):
        half = O.leaf_state_dict(scaled(cfg, sd, block, "query", 0.5), dtype=torch.float64, requires_grad=False)
        sens.append(float((decode(cfg, half, ids, enc64) - ref)[many].abs().max()))
    info = dict(peak_self=peak_self, peak_cross=peak_cross, err_ref=err_ref, sens_self=sens[0], sens_cross=sens[1],
                ratio=min(sens) / err_ref, logits=float(ref[live].abs().max()))
    if check:
        assert peak_self > PEAK and peak_cross > PEAK, info
        assert min(sens) >= RATIO * err_ref, info
    return info


def peaked(cfg, seed, px, lab):
    """-> (sd, px16, info): the sharpened state dict and pixels (bf16-exact fp32 arrays) and the figures of ``conditions`` on this
    batch plus the two query factors; both conditions asserted."""
    sd, px16, (f_self, f_cross) = sharpen(cfg, seed, px, lab)
    info = dict(factor_self=f_self, factor_cross=f_cross, **conditions(cfg, sd, px16, lab))
    return sd, px16, info


def describe(info):
    head = f"query factors {info['factor_self']:g} / {info['factor_cross']:g}, " if "factor_self" in info else ""
    return (f"{head}peaks {info['peak_self']:.2f} / {info['peak_cross']:.2f}, err_ref {info['err_ref']:.3g}, sens_self {info['sens_self']:.3g}, "
            f"sens_cross {info['sens_cross']:.3g}, min sens / err_ref {info['ratio']:.1f}, logits up to {info['logits']:.2f}")
