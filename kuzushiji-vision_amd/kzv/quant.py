"""The recipe of the e4m3 generation mode (include/kzv.h: kzv_set_decode_weights; TrOCRModel(decode_weights="e4m3")), in torch.

Per output row of a Linear's bf16 weight: s = 2^e, the smallest power of two with amax / s <= 448 (so amax / s lies in (224, 448]),
q = float8_e4m3fn(w / s), round to nearest even.  q * s has 3 mantissa bits and an exponent bf16 holds, so it IS a bf16 number, and a
power-of-two scale commutes with every fp32 rounding of a dot product: the e4m3 step computes exactly what the bf16 step computes on
the weights `dequantised_decoder_weights` returns.  Load those into any model -- this engine in bf16 mode, the HF reference, the
oracle -- to judge what the mode costs a checkpoint."""
import re

import torch

E4M3_MAX = 448.0
# the linears the one-launch generation step streams per token, by HF name below "decoder.roberta.encoder.layer.<i>." ...
LAYER_LINEARS = ("attention.self.query", "attention.self.key", "attention.self.value", "attention.output.dense",
                 "crossattention.self.query", "crossattention.output.dense", "intermediate.dense", "output.dense")
# ... and the LM head's dense layer.  NOT quantised: crossattention.self.{key,value} (once per image, a real GEMM), the tied
# vocabulary matrix, every bias and LayerNorm.
HEAD_DENSE = "decoder.lm_head.dense.weight"
_LAYER = re.compile(r"^decoder\.roberta\.encoder\.layer\.\d+\.(.+)\.weight$")


def is_quantised(name: str) -> bool:
    """Whether the e4m3 mode reads the weight of this HF name as e4m3."""
    m = _LAYER.match(name)
    return name == HEAD_DENSE or (m is not None and m.group(1) in LAYER_LINEARS)


def row_pow2_e4m3(w):
    """w [N, K] (rounded to bf16 first, as the engine's weight copies are) -> (q [N, K] torch.float8_e4m3fn, scale [N] float32), both on the host.
    The scale's exponent comes from amax's: 448 = 1.75 * 2^8, so with amax = f * 2^E, 1 <= f < 2, it is E - 8 where f <= 1.75 and
    E - 7 above; never below 2^-126; an all-zero row keeps scale 1."""
    w16 = torch.as_tensor(w).detach().to("cpu", torch.float32).to(torch.bfloat16).to(torch.float32)     # on the host: the cast is torch's CPU one
    amax = w16.abs().amax(dim=-1)
    f, e = torch.frexp(amax)                                   # amax = f * 2^e, f in [0.5, 1)
    e = torch.clamp(e - 1 - torch.where(f > 0.875, 7, 8), min=-126, max=126).to(torch.int32)
    scale = torch.where(amax > 0, torch.ldexp(torch.ones_like(amax), e), torch.ones_like(amax))
    return (w16 / scale[:, None]).to(torch.float8_e4m3fn), scale


def dequantise(q, scale):
    """q * scale as float32 (exact)."""
    return q.to(torch.float32) * scale[:, None]


def dequantised_decoder_weights(state_dict):
    """A copy of an HF-named state dict in which every weight the e4m3 mode quantises is replaced by q * s (float32 holding bf16
    values); everything else is passed through.  The e4m3 generation step equals the bf16 one on these weights bit for bit."""
    out = {}
    for k, v in state_dict.items():
        t = torch.as_tensor(v)
        out[k] = dequantise(*row_pow2_e4m3(t)).to(t.device) if is_quantised(k) and t.dim() == 2 else t.clone()
    return out
