"""Fine-tuning recipe for the ViT encoder: layer-wise learning-rate decay, a frozen bottom, no weight decay on biases and norms.

``build_groups`` is a pure function from the parameter table to the range table the grouped optimizer kernels read
(include/kzv.h: kzv_clip_and_step_groups); ``apply`` sets a model and its optimizer up from the four settings, which travel in the
checkpoint's ``hyper_parameters`` (a checkpoint without the keys means "off").

Layer ids follow the BEiT convention: 0 = encoder.patch_embeddings.*, encoder.cls_token, encoder.position_embeddings; i + 1 =
encoder.encoder.layer.i.*; Le + 1 = everything else (the encoder's final LayerNorm, encoder_decoder_proj, the decoder).
lr_scale = layer_decay ** (Le + 1 - id).
"""
from __future__ import annotations

import re

DECAY_EXEMPT = ("none", "bias_norm")
_LAYER = re.compile(r"^encoder\.encoder\.layers?\.(\d+)\.")
_NORM = re.compile(r"(layernorm|LayerNorm|layer_norm)[^.]*\.weight$")


def layer_id(name: str, enc_layers: int) -> int:
    if name.startswith("encoder.patch_embeddings.") or name in ("encoder.cls_token", "encoder.position_embeddings"):
        return 0
    m = _LAYER.match(name)
    if m:
        i = int(m.group(1))
        if i >= enc_layers:
            raise ValueError(f"{name}: layer {i} of an encoder with {enc_layers} layers")
        return i + 1
    return enc_layers + 1


def is_decay_exempt(name: str) -> bool:
    """One-dimensional parameters (biases, LayerNorm gains) and the encoder's CLS and position tables."""
    return name.endswith(".bias") or bool(_NORM.search(name)) or name in ("encoder.cls_token", "encoder.position_embeddings")


def check_settings(enc_layers: int, layer_decay: float = 1.0, freeze_encoder_layers: int = 0, decay_exempt: str = "none") -> None:
    if not 0.0 < float(layer_decay) <= 1.0:
        raise ValueError(f"layer_decay must be in (0, 1], not {layer_decay!r}")
    if isinstance(freeze_encoder_layers, bool) or int(freeze_encoder_layers) != freeze_encoder_layers or not 0 <= freeze_encoder_layers <= enc_layers:
        raise ValueError(f"freeze_encoder_layers must be an integer in 0..{enc_layers}, not {freeze_encoder_layers!r}")
    if decay_exempt not in DECAY_EXEMPT:
        raise ValueError(f"decay_exempt must be one of {DECAY_EXEMPT}, not {decay_exempt!r}")


def build_groups(param_table, enc_layers: int, layer_decay: float = 1.0, freeze_encoder_layers: int = 0, decay_exempt: str = "none"):
    """[(hf_name, offset, size)] (any order; offsets in floats, every one a multiple of 64) -> [(lo, hi, lr_scale, wd_scale)]: sorted,
    contiguous from 0 to the end of the last parameter rounded up to 64, adjacent ranges with equal scales merged.  A parameter's
    alignment padding joins its own range.  Freezing n > 0 layers gives lr_scale 0 exactly to ids 0..n."""
    check_settings(enc_layers, layer_decay, freeze_encoder_layers, decay_exempt)
    rows = sorted((int(off), int(size), str(name)) for name, off, size in param_table)
    if not rows or rows[0][0] != 0:
        raise ValueError("the parameter table must start at offset 0")
    out: list[list] = []
    for j, (off, size, name) in enumerate(rows):
        end = rows[j + 1][0] if j + 1 < len(rows) else (off + size + 63) // 64 * 64
        if off % 64 or size < 1 or off + size > end:
            raise ValueError(f"{name}: [{off}, {off + size}) is not 64-aligned or overlaps the next parameter")
        lid = layer_id(name, enc_layers)
        frozen = freeze_encoder_layers > 0 and lid <= freeze_encoder_layers
        lr_scale = 0.0 if frozen else float(layer_decay) ** (enc_layers + 1 - lid)
        wd_scale = 0.0 if decay_exempt == "bias_norm" and is_decay_exempt(name) else 1.0
        if out and out[-1][2] == lr_scale and out[-1][3] == wd_scale:
            out[-1][1] = end
        else:
            out.append([off, end, lr_scale, wd_scale])
    return [tuple(g) for g in out]


def model_param_table(cfg):
    """[(hf_name, offset, size)] of a TrOCR configuration: one entry per reference state_dict key (tied aliases left out), the
    offsets of kzv_param_info plus the key's place inside a fused block (Q/K/V, the decoder's cross-attention K/V)."""
    from . import params as P
    offs, _ = P.param_offsets(cfg)
    table = []
    for hf, eng, rel, shape in P.hf_views(cfg):
        if hf in P.TIED_ALIASES:
            continue
        n = 1
        for d in shape:
            n *= int(d)
        table.append((hf, offs[eng][0] + rel, n))
    return table


def summary(groups) -> str:
    """One line for the log: group count, smallest and largest scale of the trainable groups, frozen and trainable floats."""
    frozen = sum(hi - lo for lo, hi, ls, _ in groups if ls == 0.0)
    train = sum(hi - lo for lo, hi, ls, _ in groups if ls != 0.0)
    scales = [ls for _, _, ls, _ in groups if ls != 0.0] or [0.0]
    exempt = sum(hi - lo for lo, hi, ls, ws in groups if ls != 0.0 and ws == 0.0)
    return (f"parameter groups: {len(groups)}, lr scale {min(scales):.4g} .. {max(scales):.4g}, frozen {frozen:,} / trainable {train:,} "
            f"parameters (aligned), {exempt:,} without weight decay")


def is_default(layer_decay: float = 1.0, freeze_encoder_layers: int = 0, decay_exempt: str = "none") -> bool:
    return float(layer_decay) == 1.0 and int(freeze_encoder_layers) == 0 and decay_exempt == "none"


def settings_from_hparams(hp) -> dict:
    """The four settings as a checkpoint's ``hyper_parameters`` (a dict or a namespace, possibly None) record them; a checkpoint
    without the keys -- every reference checkpoint, every earlier one of this engine -- means "off"."""
    def get(name, default):
        if hp is None:
            return default
        return hp.get(name, default) if isinstance(hp, dict) else getattr(hp, name, default)
    return {"layer_decay": float(get("layer_decay", 1.0)), "freeze_encoder_layers": int(get("frozen_encoder_layers", 0)),
            "decay_exempt": str(get("decay_exempt", "none")), "accumulate_grad_batches": int(get("accumulate_grad_batches", 1))}


def apply(model, opt, layer_decay: float = 1.0, freeze_encoder_layers: int = 0, decay_exempt: str = "none"):
    """Set the model's frozen layers and the optimizer's groups from the settings and record them in the model's hparams.  With every
    setting at its default the optimizer keeps the plain kernels (set_groups(None)).  Returns the group table or None."""
    check_settings(model.cfg.enc_layers, layer_decay, freeze_encoder_layers, decay_exempt)
    model.frozen_encoder_layers = int(freeze_encoder_layers)
    model.hparams.layer_decay, model.hparams.decay_exempt = float(layer_decay), decay_exempt
    groups = None
    if not is_default(layer_decay, freeze_encoder_layers, decay_exempt):
        groups = build_groups(model_param_table(model.cfg), model.cfg.enc_layers, layer_decay, int(freeze_encoder_layers), decay_exempt)
        total = model.flat_params.numel()
        if groups[-1][1] != total:
            raise ValueError(f"the parameter table ends at {groups[-1][1]}, the flat buffer has {total} floats")
    if opt is not None:
        opt.set_groups(groups)
    return groups
