"""Host-side mirror of the reference's ``TrOCRModel`` (src/models/trocr_model.py:205-460).

Same constructor, same ``forward`` contract, same step / hook / utility methods, same ``state_dict`` key
names -- but every FLOP runs in libkzv's hand-written HIP kernels through the C ABI of include/kzv.h.
torch is used for device memory, streams and (in kzv.trainer) torch.distributed only; there is no
autograd and no fallback path.
"""
from __future__ import annotations

import contextlib
import ctypes as C
import itertools
import os
import types
from typing import Any

from . import _lib as L
from . import params as P
from .config import ModelConfig, load_decoder_config


class _Cfg(types.SimpleNamespace):
    pass


def encoder_attention_impl(cfg: ModelConfig, long_sequences: bool = False) -> str:
    """Which attention kernels the encoder of `cfg` runs on, forward and backward: "mfma64" | "mfma96" | "valu", and for a
    model built with long_sequences also "stream64" | "stream96" (kzv_attn_impl / kzv_attn_impl_ex: no GPU needed)."""
    hd, S = cfg.enc_hidden // cfg.enc_heads, cfg.enc_seq
    fwd = L.attention_impl(hd, S, S, heads=cfg.enc_heads, long_sequences=long_sequences)
    bwd = L.attention_impl(hd, S, S, heads=cfg.enc_heads, bwd=True, long_sequences=long_sequences)
    assert fwd == bwd, (fwd, bwd)
    return fwd


class TrOCRModel:
    """TrOCR Model with ViT Encoder and RoBERTa Decoder (MI355X engine).

    Mirrors src/models/trocr_model.py:208-217 (constructor), :258-321 (forward), :323-460 (steps, CER,
    optimizer, mode hooks, decode_predictions).
    """

    def __init__(self, encoder_config: dict[str, Any], decoder_path: str, learning_rate: float = 1e-4,
                 beta1: float = 0.9, beta2: float = 0.999, epsilon: float = 1e-8, weight_decay: float = 0,
                 *, device: str = "cuda", init_seed: int = 42, load_tokenizer: bool = True, width_buckets=None,
                 fp8: bool = False, long_sequences: bool = False, decode_weights: str = "bf16", label_smoothing: float = 0.0,
                 class_weights=None, focal_gamma: float = 0.0):
        import torch
        self._check_label_smoothing(label_smoothing)
        self._check_focal_gamma(focal_gamma, label_smoothing)
        self.hparams = types.SimpleNamespace(encoder_config=encoder_config, decoder_path=decoder_path,
                                             learning_rate=learning_rate, beta1=beta1, beta2=beta2,
                                             epsilon=epsilon, weight_decay=weight_decay, label_smoothing=float(label_smoothing),
                                             class_weights=None, focal_gamma=0.0,
                                             # fine-tuning (kzv/finetune.py); the defaults are "off", and a checkpoint without the keys loads as such
                                             frozen_encoder_layers=0, layer_decay=1.0, decay_exempt="none", accumulate_grad_batches=1)
        dec_cfg = load_decoder_config(decoder_path)          # FileNotFoundError like scripts/train_trocr.py:88-89
        self.cfg = ModelConfig.from_reference(encoder_config, dec_cfg)
        # long_sequences (include/kzv.h: KZV_MODEL_LONG_SEQ): encoders with head_dim 64 or 96 take up to 4,097 tokens, attention
        # launches beyond 288 tokens running the K/V-streaming kernels.  Off by default: the library keeps the 288-token cap.
        self.long_sequences = bool(long_sequences)
        self.cfg.validate(long_sequences=self.long_sequences)
        self.tokenizer = None
        if load_tokenizer:
            from transformers import AutoTokenizer                      # trocr_model.py:222
            self.tokenizer = AutoTokenizer.from_pretrained(decoder_path)
        # attribute surface used by scripts/test_trocr_setup.py:118-120
        self.encoder = types.SimpleNamespace(config=_Cfg(hidden_size=self.cfg.enc_hidden), num_patches=self.cfg.num_patches)
        self.decoder = types.SimpleNamespace(config=_Cfg(hidden_size=self.cfg.dec_hidden, vocab_size=self.cfg.vocab))
        self.training = True
        self.device = torch.device(device)
        self.logged: dict[str, list[float]] = {}
        self._optimizer = None
        self._step_seed = 0
        self.trim_padding = True
        self._len_cache = (None, 0)
        self._keep = None                  # inputs of the last engine call (kept alive; align_last reads the labels)
        self.last_active_length = 0
        self.last_stream_steps = 0
        self.last_generate_steps = 0
        self.last_stream_pad_fallbacks = 0
        self._stream_beams = 4
        # what lockstep ``generate`` runs for its generation controls: "device" (kzv_logits_process) or "reference" (the torch statement
        # kzv/controls.py::process_reference on the same step scores; the tests' cross-check, far slower)
        self.controls_impl = "device"
        # the same switch for the language-model fusion of lockstep ``generate``: "device" (kzv_lm_fuse) or "reference" (kzv/lm.py::fuse_reference)
        self.lm_impl = "device"
        # and for the forced prefixes of lockstep ``generate``: "device" (kzv_force_prefix) or "reference" (kzv/prefix.py::force_reference)
        self.prefix_impl = "device"
        # generation controls of the validation / test decodes (``forward`` without labels): generate's keywords; empty = the reference's
        self.decode_controls = {}
        # Width buckets (BASELINE.json configs[4]; an extension -- a reference model has one image size): encoder_config's
        # image_size is the WIDEST crop; batches whose width is one of `width_buckets` (multiples of the patch width, <= it)
        # run with fewer patch tokens and the position rows of the same (h, w) cells (include/kzv.h: kzv_set_image_width).
        self.width_buckets = tuple(sorted(int(w) for w in width_buckets)) if width_buckets else None
        if self.width_buckets:
            for w in self.width_buckets:
                if w % self.cfg.patch_w or not (self.cfg.patch_w <= w <= self.cfg.image_w):
                    raise ValueError(f"width bucket {w} must be a multiple of {self.cfg.patch_w} and <= {self.cfg.image_w}")

        lib = L.load()
        c = self.cfg
        self._ccfg = L.kzv_config(
            image_h=c.image_h, image_w=c.image_w, patch_h=c.patch_h, patch_w=c.patch_w, channels=c.channels,
            enc_hidden=c.enc_hidden, enc_layers=c.enc_layers, enc_heads=c.enc_heads, enc_ffn=c.enc_ffn,
            dec_hidden=c.dec_hidden, dec_layers=c.dec_layers, dec_heads=c.dec_heads, dec_ffn=c.dec_ffn,
            vocab=c.vocab, max_pos=c.max_pos, type_vocab=c.type_vocab, pad_id=c.pad_id,
            enc_hidden_dropout=c.enc_hidden_dropout, enc_attn_dropout=c.enc_attn_dropout,
            dec_hidden_dropout=c.dec_hidden_dropout, dec_attn_dropout=c.dec_attn_dropout, ln_eps=c.ln_eps)
        h = C.c_void_p()
        if self.long_sequences:
            L.check(lib.kzv_model_create_ex(C.byref(self._ccfg), L.MODEL_LONG_SEQ, C.byref(h)), "kzv_model_create_ex")
        else:
            L.check(lib.kzv_model_create(C.byref(self._ccfg), C.byref(h)), "kzv_model_create")
        self._h = h
        # fp8 weight path (BASELINE.json configs[4]; an extension -- the reference trains in bf16 autocast): the encoder's QKV,
        # fc1 and fc2 forward GEMMs read e4m3 weights and activations (include/kzv.h: kzv_set_fp8); backward stays bf16.
        # fp8 = True / 1: forward GEMMs; 2: also the MLP's two input-gradient GEMMs
        self.fp8 = int(fp8)
        if self.fp8:
            L.check(lib.kzv_set_fp8(h, self.fp8), "kzv_set_fp8")
        # generation from e4m3 decoder weights (an extension; include/kzv.h: kzv_set_decode_weights, kzv/quant.py): opt-in, and only
        # where the one-launch step runs -- decode_weights_impl says what a generate actually read
        self.set_decode_weights(decode_weights)
        # label smoothing of the TRAINING loss (an extension; include/kzv.h: kzv_set_label_smoothing): F.cross_entropy(label_smoothing=eps)
        # inside the loss kernels; evaluation forwards (val_loss, test) keep the plain loss.  0 = the reference's criterion.
        self.label_smoothing = label_smoothing
        # class weights and the focal term of the TRAINING loss (extensions; include/kzv.h: kzv_set_class_weights states both losses):
        # F.cross_entropy(weight=w) and (1 - p_t)^gamma inside the loss kernels; evaluation forwards keep the plain loss.  None / 0 = off.
        self.class_weights = class_weights
        self.focal_gamma = focal_gamma
        self._offsets, total = P.param_offsets(c)
        if lib.kzv_param_total(h) != total:
            raise L.KzvError("parameter table mismatch between kzv/params.py and libkzv")
        self.flat_params = torch.zeros(total, dtype=torch.float32, device=self.device)
        self.flat_grads = torch.zeros(total, dtype=torch.float32, device=self.device)
        self._ws = None
        self._bound = (0, 0)
        self._loss = torch.zeros(1, dtype=torch.float32, device=self.device)
        # seeded init (the reference seeds 42: scripts/train_trocr.py:78); weights arrive via load_state_dict
        self.flat_params.copy_(torch.from_numpy(P.recipe_flat(c, init_seed)))
        # decoder weights from decoder_path if present (AutoModelForCausalLM.from_pretrained, trocr_model.py:231)
        self._maybe_load_decoder_weights(decoder_path)

    # ------------------------------------------------------------------ plumbing
    def __del__(self):
        try:
            if getattr(self, "_h", None):
                L.load().kzv_model_destroy(self._h)
                self._h = None
        except Exception:
            pass

    def _maybe_load_decoder_weights(self, path: str) -> None:
        f = os.path.join(path, "model.safetensors")
        if not os.path.exists(f):
            return
        from safetensors.torch import load_file
        sd = load_file(f)
        mine = self.state_dict_views()
        for k, v in sd.items():
            name = "decoder." + k
            if name in mine and tuple(mine[name].shape) == tuple(v.shape):
                mine[name].copy_(v.to(self.device, dtype=mine[name].dtype))

    def fp8_act_scales(self):
        """Per-layer multipliers the last forward quantised the encoder's GELU outputs with (parity hook)."""
        import torch
        out = torch.empty(self.cfg.enc_layers, dtype=torch.float32, device=self.device)
        L.check(L.load().kzv_fp8_act_scales(self._h, out.data_ptr(), L.stream_handle()), "kzv_fp8_act_scales")
        torch.cuda.synchronize()
        return out.cpu()

    def _bind(self, batch: int, label_len: int) -> None:
        import torch
        if self._bound == (batch, label_len):
            return
        lib = L.load()
        need = lib.kzv_workspace_bytes(self._h, batch, label_len)
        if need < 0:
            L.check(-1, "kzv_workspace_bytes")
        if self._ws is None or self._ws.numel() < need:
            self._ws = None
            self._ws = torch.empty(need, dtype=torch.uint8, device=self.device)
        L.check(lib.kzv_model_bind(self._h, self.flat_params.data_ptr(), self.flat_grads.data_ptr(),
                                   self._ws.data_ptr(), self._ws.numel(), batch, label_len), "kzv_model_bind")
        self._bound = (batch, label_len)
        self.sync_weights()

    def sync_weights(self) -> None:
        if self._bound != (0, 0):
            L.check(L.load().kzv_model_sync_weights(self._h, L.stream_handle()), "sync_weights")

    def zero_grad(self) -> None:
        self.flat_grads.zero_()

    # ------------------------------------------------------------------ nn.Module-like surface
    def state_dict_views(self):
        """HF-named views into the flat master buffer (writing through them edits the model)."""
        return P.state_dict_from_flat(self.cfg, self.flat_params)

    def state_dict(self):
        return {k: v.detach().clone() for k, v in self.state_dict_views().items()}

    def grad_dict(self):
        return {k: v for k, v in P.state_dict_from_flat(self.cfg, self.flat_grads).items()}

    def load_state_dict(self, sd, strict: bool = True):
        import torch
        mine = self.state_dict_views()
        seen = set()
        for k, v in sd.items():
            name = P.canonical_hf_name(k)
            if name not in mine:
                if strict:
                    raise KeyError(f"unexpected key {k}")
                continue
            t = torch.as_tensor(v)
            if tuple(t.shape) != tuple(mine[name].shape):
                raise ValueError(f"size mismatch for {k}: {tuple(t.shape)} vs {tuple(mine[name].shape)}")
            mine[name].copy_(t.to(self.device, dtype=torch.float32))
            seen.add(name)
        if strict:
            missing = [k for k in mine if k not in seen and k not in P.TIED_ALIASES]
            if missing:
                raise KeyError(f"missing keys: {missing[:4]}...")
        self.sync_weights()
        if self._optimizer is not None:
            self._optimizer.z.copy_(self.flat_params)

    def parameters(self):
        return [self.flat_params]

    def num_parameters(self) -> int:
        return P.num_parameters(self.cfg)

    @property
    def encoder_attention_impl(self) -> str:
        """"mfma64" | "mfma96" | "valu" | "stream64" | "stream96": the attention kernels of this model's encoder (at its
        widest crop)."""
        return encoder_attention_impl(self.cfg, self.long_sequences)

    @property
    def decode_step_impl(self) -> str:
        """"one-launch" | "per-operation": how the next KV-cached generation step of this model runs (kzv_decode_step_impl: the
        bound rows, the images and crop width of the last generate, the kzv_set_decode_one_launch mode).  Valid once a generate
        (or _bind) has bound the model; before the first encoder pass it answers "per-operation"."""
        rc = L.load().kzv_decode_step_impl(self._h)
        if rc < 0:
            L.check(rc, "kzv_decode_step_impl")
        return "one-launch" if rc == 1 else "per-operation"

    _DECODE_WEIGHTS = ("bf16", "e4m3")

    def set_decode_weights(self, fmt: str) -> None:
        """"bf16" (default) | "e4m3": what the KV-cached generation steps after this call read the decoder's streamed linears as."""
        if fmt not in self._DECODE_WEIGHTS:
            raise ValueError(f"decode_weights must be one of {self._DECODE_WEIGHTS}, not {fmt!r}")
        L.check(L.load().kzv_set_decode_weights(self._h, self._DECODE_WEIGHTS.index(fmt)), "kzv_set_decode_weights")
        self.decode_weights = fmt

    @property
    def decode_weights_impl(self) -> str:
        """"bf16" | "e4m3": what the next KV-cached generation step of this model will actually read (kzv_decode_weights_impl): "e4m3"
        only where it was asked for and decode_step_impl is "one-launch".  Valid when decode_step_impl is."""
        rc = L.load().kzv_decode_weights_impl(self._h)
        if rc < 0:
            L.check(rc, "kzv_decode_weights_impl")
        return self._DECODE_WEIGHTS[rc]

    @staticmethod
    def _check_label_smoothing(eps) -> None:
        if not 0.0 <= float(eps) < 1.0:
            raise ValueError(f"label_smoothing must be in [0, 1), not {eps!r}")

    @property
    def label_smoothing(self) -> float:
        """eps of the training loss, F.cross_entropy(..., label_smoothing=eps).  Training-mode forwards only: eval-mode forwards return
        the plain loss whatever it is.  Setting it (kzv_set_label_smoothing) takes effect on the next forward and is recorded in hparams,
        which is what this returns: the value as given, of which the handle holds the fp32 rounding (kzv_get_label_smoothing)."""
        return self.hparams.label_smoothing

    @label_smoothing.setter
    def label_smoothing(self, eps: float) -> None:
        self._check_label_smoothing(eps)
        if float(eps) > 0.0 and self.hparams.focal_gamma > 0.0:
            raise ValueError(f"label_smoothing {eps!r} with focal_gamma {self.hparams.focal_gamma!r}: no such loss is stated; set one of them to 0")
        L.check(L.load().kzv_set_label_smoothing(self._h, float(eps)), "kzv_set_label_smoothing")
        self.hparams.label_smoothing = float(eps)

    @property
    def frozen_encoder_layers(self) -> int:
        """Frozen bottom of the encoder, 0 <= n <= encoder layers (0: everything trains).  n > 0 freezes the patch embedding, the CLS token, the
        position table and encoder layers 0 .. n-1: the backward launches nothing for them (kzv_set_frozen_encoder_layers) and their
        gradients stay zero.  The optimizer is told separately (kzv.finetune.apply gives the same ranges lr_scale 0).  Recorded in hparams."""
        return self.hparams.frozen_encoder_layers

    @frozen_encoder_layers.setter
    def frozen_encoder_layers(self, n: int) -> None:
        if isinstance(n, bool) or int(n) != n or not 0 <= int(n) <= self.cfg.enc_layers:
            raise ValueError(f"frozen_encoder_layers must be an integer in 0..{self.cfg.enc_layers}, not {n!r}")
        L.check(L.load().kzv_set_frozen_encoder_layers(self._h, int(n)), "kzv_set_frozen_encoder_layers")
        self.hparams.frozen_encoder_layers = int(n)

    @staticmethod
    def _check_focal_gamma(gamma, eps) -> None:
        if not 0.0 <= float(gamma) <= 5.0:
            raise ValueError(f"focal_gamma must be in [0, 5], not {gamma!r}")
        if float(gamma) > 0.0 and float(eps) > 0.0:
            raise ValueError(f"focal_gamma {gamma!r} with label_smoothing {eps!r}: no such loss is stated; set one of them to 0")

    @property
    def focal_gamma(self) -> float:
        """gamma of the focal modulation (1 - p_t)^gamma of the training loss, 0 <= gamma <= 5 (0: off), only with label_smoothing 0.
        Training-mode forwards only, like label_smoothing; recorded in hparams (kzv_set_focal_gamma)."""
        return self.hparams.focal_gamma

    @focal_gamma.setter
    def focal_gamma(self, gamma: float) -> None:
        self._check_focal_gamma(gamma, self.hparams.label_smoothing)
        L.check(L.load().kzv_set_focal_gamma(self._h, float(gamma)), "kzv_set_focal_gamma")
        self.hparams.focal_gamma = float(gamma)

    @property
    def class_weights(self):
        """Per-class weights of the training loss, F.cross_entropy(weight=w): a float32 CPU tensor [vocab], or None (off).  Accepts a tensor,
        an ndarray or a list of length vocab, every value finite and > 0.  Training-mode forwards only; the loss and every gradient are
        normalised by the sum of the targets' weights, as torch does.  Recorded in hparams (kzv_set_class_weights copies the values)."""
        return self.hparams.class_weights

    @class_weights.setter
    def class_weights(self, w) -> None:
        import torch
        lib = L.load()
        if w is None:
            L.check(lib.kzv_set_class_weights(self._h, None, 0), "kzv_set_class_weights")
            self.hparams.class_weights = None
            return
        t = torch.as_tensor(w).detach().to(device="cpu", dtype=torch.float32).contiguous().clone()
        if t.dim() != 1 or t.numel() != self.cfg.vocab:
            raise ValueError(f"class_weights must hold {self.cfg.vocab} values (the vocabulary), not shape {tuple(t.shape)}")
        if not bool(torch.isfinite(t).all()) or not bool((t > 0).all()):
            raise ValueError("class_weights must be finite and > 0")
        L.check(lib.kzv_set_class_weights(self._h, t.data_ptr(), t.numel()), "kzv_set_class_weights")
        self.hparams.class_weights = t

    def train(self, mode: bool = True):
        self.training = mode
        return self

    def eval(self):
        return self.train(False)

    def to(self, device):
        return self

    def log(self, name, value, sync_dist: bool = False, **kw):
        """LightningModule.log: the reference logs train_loss / val_loss / val_cer / test_* WITHOUT sync_dist
        (trocr_model.py:331,342,358,370,388), i.e. each rank's own value and rank 0's in the logger -- the default here.
        sync_dist=True is Lightning's mean over ranks: one scalar all-reduce."""
        v = float(value)
        if sync_dist:
            import torch
            import torch.distributed as dist
            if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
                t = torch.tensor([v], dtype=torch.float64, device=self.device if dist.get_backend() == "nccl" else "cpu")
                dist.all_reduce(t, op=dist.ReduceOp.SUM)
                v = float(t.item()) / dist.get_world_size()
        self.logged.setdefault(name, []).append(v)

    def optimizers(self):
        return self._optimizer

    def __call__(self, pixel_values, labels=None):
        return self.forward(pixel_values, labels)

    # ------------------------------------------------------------------ forward (trocr_model.py:258-321)
    def _check_inputs(self, pixel_values):
        import torch
        c = self.cfg
        if pixel_values.dim() != 4 or pixel_values.shape[1] != c.channels:
            raise ValueError(f"pixel_values must be [B,{c.channels},H,W], got {tuple(pixel_values.shape)}")
        _, _, height, width = pixel_values.shape
        bucket_ok = self.width_buckets is not None and width in self.width_buckets
        if height != c.image_h or (width != c.image_w and not bucket_ok):   # trocr_model.py:83-86
            raise ValueError(f"Input image size ({height}*{width}) doesn't match model ({c.image_h}*{c.image_w}).")
        L.check(L.load().kzv_set_image_width(self._h, int(width)), "set_image_width")
        return pixel_values.to(self.device, dtype=torch.float32).contiguous()

    def forward_loss(self, pixel_values, labels, want_logits: bool = False, seed: int | None = None):
        """Engine call: returns (loss tensor [1] on device, logits or None).  Dropout follows self.training."""
        import torch
        px = self._check_inputs(pixel_values)
        n_max_host = None
        if labels.device.type == "cpu" and labels.dim() == 2:      # dataloader batches: length known without touching the GPU
            n_max_host = int((labels != self.cfg.pad_id).sum(dim=1).max())
            # RoBERTa position ids run to (non-pad decoder inputs) + pad_id and index a [max_pos, H] table
            # (HF modeling_roberta.py:142-155): a longer label raises in the reference ("index out of range in self")
            n_in = int((labels[:, :-1] != self.cfg.pad_id).sum(dim=1).max()) if labels.shape[1] > 1 else 0
            if n_in + self.cfg.pad_id >= self.cfg.max_pos:
                raise IndexError(f"index out of range in self: {n_in} decoder input tokens need position id {n_in + self.cfg.pad_id}, "
                                 f"the position table has {self.cfg.max_pos} rows")
        lab = labels.to(self.device, dtype=torch.int64).contiguous()
        if lab.dim() != 2 or lab.shape[0] != px.shape[0]:
            raise ValueError("labels must be [B, L]")
        B, Lh = lab.shape
        self._bind(B, Lh)
        logits = torch.empty(B, Lh - 1, self.cfg.vocab, dtype=torch.float32, device=self.device) if want_logits else None
        if seed is None:
            self._step_seed += 1
            seed = self._step_seed
        self._keep = (px, lab)   # inputs must outlive the asynchronous kernels (and backward reads labels)
        # trailing all-padding decoder positions change neither loss nor gradients: run the decoder on the prefix that
        # holds characters (one tiny device reduction + sync per step; full length when logits are returned)
        t_act = Lh - 1
        if not want_logits and self.trim_padding:
            key = (lab.data_ptr(), lab._version, tuple(lab.shape))
            if n_max_host is not None:
                n_max = n_max_host
            elif self._len_cache[0] == key:                       # same resident batch again (benchmark loop): no sync
                n_max = self._len_cache[1]
            else:
                n_max = int((lab != self.cfg.pad_id).sum(dim=1).max().item())
                self._len_cache = (key, n_max)
            t_act = max(1, min(Lh - 1, n_max))
        self.last_active_length = t_act
        L.check(L.load().kzv_set_active_length(self._h, t_act), "set_active_length")
        L.check(L.load().kzv_forward_loss(self._h, px.data_ptr(), lab.data_ptr(), self._loss.data_ptr(), L.ptr(logits),
                                          1 if self.training else 0, seed, L.stream_handle()), "kzv_forward_loss")
        return self._loss, logits

    def forward(self, pixel_values, labels=None):
        if labels is not None:
            loss, logits = self.forward_loss(pixel_values, labels, want_logits=True)
            return {"logits": logits, "loss": loss.clone().reshape(())}
        # trocr_model.py:306-316: max_length=128, num_beams=4, early_stopping=True
        return {"generated_ids": self.generate(pixel_values, max_length=128, num_beams=4, early_stopping=True, **self.decode_controls),
                "logits": None}

    def backward(self, accumulate: bool = False) -> None:
        """loss.backward() of the last training-mode forward: fills flat_grads (zeroed first).  ``accumulate`` skips the zeroing, so the
        pass adds to what the buffer holds (every gradient kernel adds: DESIGN.md section 7)."""
        lib = L.load()
        st = L.stream_handle()
        if not accumulate:
            L.check(lib.kzv_zero_grads(self._h, st), "zero_grads")
        L.check(lib.kzv_backward(self._h, st), "kzv_backward")

    # ------------------------------------------------------------------ per-character confidence and position
    def align_last(self, layer=-1, want_map: bool = False, top_k: int = 0):
        """Scores and cross-attention of the LAST ``forward_loss`` / ``forward(pixel_values, labels)`` on this model, read back from
        its saved activations (kzv_score_tokens, kzv_cross_attention); see ``align`` for the result.  Raises KzvError when a
        generate, a rebind or a change of geometry has replaced those activations.  A pending ``backward`` still works.  ``top_k`` in
        1..8 adds ``alt_ids`` / ``alt_logprob`` (kzv_score_tokens_topk)."""
        import torch
        from . import align as A
        c = self.cfg
        top_k = int(top_k)
        if not 0 <= top_k <= 8:
            raise ValueError("top_k must be in 0..8")
        lib = L.load()
        st = L.stream_handle()
        if self._keep is None:
            raise L.KzvError("align_last: no forward_loss has run on this model")
        px, lab = self._keep
        B, Lh = lab.shape
        Ta = self.last_active_length
        grid_w = px.shape[3] // c.patch_w
        n_patches = (c.image_h // c.patch_h) * grid_w
        layers = [layer] if isinstance(layer, int) else [int(x) for x in layer]
        if not layers:
            raise ValueError("layer: an int or a non-empty sequence of ints")
        for x in layers:
            if not -c.dec_layers <= x < c.dec_layers:
                raise ValueError(f"layer {x} outside -{c.dec_layers}..{c.dec_layers - 1}")
        layers = [x % c.dec_layers for x in layers]
        dev = self.device
        logprob = torch.empty(B, Ta, dtype=torch.float32, device=dev)
        top1 = torch.empty(B, Ta, dtype=torch.int64, device=dev)
        top1_lp = torch.empty(B, Ta, dtype=torch.float32, device=dev)
        L.check(lib.kzv_score_tokens(self._h, logprob.data_ptr(), top1.data_ptr(), top1_lp.data_ptr(), st), "kzv_score_tokens")
        pos = torch.empty(B, Ta, 4, dtype=torch.float32, device=dev)
        peak = torch.empty(B, Ta, dtype=torch.int32, device=dev)
        amap = None
        need_map = want_map or len(layers) > 1
        for i, x in enumerate(layers):
            m_i = torch.empty(B, Ta, n_patches, dtype=torch.float32, device=dev) if need_map else None
            L.check(lib.kzv_cross_attention(self._h, x, L.ptr(m_i), n_patches, pos.data_ptr(), peak.data_ptr(), st), "kzv_cross_attention")
            if need_map:
                amap = m_i if amap is None else amap.add_(m_i)
        if len(layers) > 1:                                   # the mean map of several layers: centroid / peak restated in torch
            amap = amap / len(layers)
            pos, peak = A.stats_from_map(amap, grid_w)
        T = Lh - 1
        out = {
            "logprob": A.pad_rows(logprob, T), "top1": A.pad_rows(top1, T, c.pad_id), "top1_logprob": A.pad_rows(top1_lp, T),
            "centroid": A.pad_rows(A.patch_to_pixel(pos[..., :2], c.patch_h, c.patch_w), T),
            "peak_patch": A.pad_rows(peak, T), "peak_weight": A.pad_rows(pos[..., 2].contiguous(), T),
            "row_sum": A.pad_rows(pos[..., 3].contiguous(), T),
            "live": A.live_mask(lab, c.pad_id),
        }
        if want_map:
            out["map"] = A.pad_rows(amap, T)
        if top_k:
            alt_ids = torch.empty(B, Ta, top_k, dtype=torch.int32, device=dev)
            alt_lp = torch.empty(B, Ta, top_k, dtype=torch.float32, device=dev)
            L.check(lib.kzv_score_tokens_topk(self._h, top_k, alt_ids.data_ptr(), alt_lp.data_ptr(), st), "kzv_score_tokens_topk")
            out["alt_ids"] = A.pad_rows(alt_ids.long(), T, -1)
            out["alt_logprob"] = A.pad_rows(alt_lp, T)
        return out

    def align(self, pixel_values, labels, layer=-1, want_map: bool = False, top_k: int = 0):
        """Per-position confidence and position of ``labels`` [B, L] on the crops: one eval-mode teacher-forced pass (no logits
        are materialised for the caller; trailing padding is trimmed as in training), then the two read-backs.  Returns device
        tensors padded back to [B, L - 1]; row t belongs to the token labels[:, t + 1]:

          logprob, top1, top1_logprob   log-softmax at the label, the arg-max token and its log-probability
          centroid [B, L - 1, 2]        attention centroid (y, x) in pixels: ((row + 0.5) * patch_h, (col + 0.5) * patch_w)
          peak_patch, peak_weight       the arg-max patch of the head-averaged cross-attention and its weight
          row_sum                       the sum of the weights (1 up to rounding: a health value)
          map [B, L - 1, n_patches]     the weights themselves, when ``want_map``
          live                          decoder input and target both non-pad (other rows are padding or zeros)
          alt_ids, alt_logprob [B, L - 1, k]  with ``top_k`` = k in 1..8: the k best tokens of every position and their
                                        log-probabilities, best first, ties by the smaller id (entry 0 = top1 / top1_logprob; HF:
                                        output_scores=True, scores[t].log_softmax(-1).topk(k)); -1 / 0 in the trimmed padding

        ``layer``: a decoder layer (negative from the end) or a sequence of them, whose maps are averaged (HF:
        ``cross_attentions[layer].mean(1)``)."""
        was = self.training
        self.training = False
        try:
            self.forward_loss(pixel_values, labels, want_logits=False, seed=0)
        finally:
            self.training = was
        return self.align_last(layer, want_map, top_k)

    def recognize(self, pixel_values, num_beams: int = 4, max_length: int = 128, layer=-1, top_k: int = 0,
                  no_repeat_ngram_size: int = 0, repetition_penalty: float = 1.0, min_length: int = 0, suppress_tokens=None,
                  allowed_tokens=None, lm=None, lm_weight: float = 0.0, n_best: int = 0, prefix_ids=None, prefix_texts=None) -> list[dict]:
        """``generate`` (the reference's settings: beam 4, max_length 128, early stopping), then ``align`` with the generated
        ids as labels: per image a dict of ``text``, ``tokens`` (ids without BOS / EOS / PAD), ``token_strings``,
        ``logprobs``, ``confidence`` = exp(mean log-probability over the tokens, EOS included), ``centroids`` ((y, x) in
        pixels) and ``peak_patches`` (kzv/align.py: build_records).  ``top_k`` in 1..8 adds ``alternatives`` (per token the k best
        candidates of the teacher-forced pass with their log-probabilities) and ``margins``; after a beam search the chosen token
        need not be the first alternative.  The generation controls are ``generate``'s and steer the decode only: the align-based
        values (log-probabilities, confidence, alternatives) stay the model's own, so a token the controls forced may carry a low one.
        ``lm`` / ``lm_weight`` (``generate``'s language-model fusion) do the same: they steer the decode only.
        ``n_best`` n in 1..num_beams: every record also holds ``score`` (HF ``sequences_scores``) and ``hypotheses``, the n best readings
        of the line as ``recognize_many``'s records (the search's own log-probabilities, best first, entry 0 the winner's reading); the
        align pass still supplies centroids, log-probabilities and confidence of the winner only.
        ``prefix_ids`` (``generate``'s forced prefixes) or ``prefix_texts`` (a list of strings, through the tokenizer; one-character
        tokenizers only): the first characters of every line are given and the model reads the rest.  Every record then holds
        ``forced`` (how many tokens were given); ``confidence`` is taken over the free tokens only, and the ``alternatives`` of forced
        positions are empty.  ``logprobs`` stay the model's own opinion of every token, forced ones included (the align pass)."""
        import torch
        from . import align as A
        from . import prefix as PF
        c = self.cfg
        if prefix_texts is not None:
            if prefix_ids is not None:
                raise ValueError("recognize: prefix_ids or prefix_texts, not both")
            prefix_ids = PF.texts_to_ids(self.tokenizer, prefix_texts)
        forced = None
        if prefix_ids is not None:
            got = PF.normalise(prefix_ids, len(prefix_ids), vocab=c.vocab, pad_id=c.pad_id, bos_id=c.bos_id, eos_id=c.eos_id,
                               max_length=min(max_length, c.max_pos - c.pad_id - 1))
            forced = [0] * len(prefix_ids) if got is None else got[1].tolist()
        hyps = None
        if n_best:
            from . import nbest as NB
            n = NB.check_request(num_beams, n_best, True, "recognize")
            gen_all, h_sc, h_lp = self.generate(pixel_values, max_length=max_length, num_beams=num_beams, early_stopping=True,
                                                no_repeat_ngram_size=no_repeat_ngram_size, repetition_penalty=repetition_penalty, min_length=min_length,
                                                suppress_tokens=suppress_tokens, allowed_tokens=allowed_tokens, lm=lm, lm_weight=lm_weight,
                                                num_return_sequences=n, return_scores=True, return_logprobs=True, prefix_ids=prefix_ids)
            hyps = NB.records(self, gen_all, h_sc, h_lp, n)
            gen = gen_all[0::n]
            gen = gen[:, :max(1, int((gen != c.pad_id).sum(dim=1).max()))]
        else:
            gen = self.generate(pixel_values, max_length=max_length, num_beams=num_beams, early_stopping=True,
                                no_repeat_ngram_size=no_repeat_ngram_size, repetition_penalty=repetition_penalty, min_length=min_length,
                                suppress_tokens=suppress_tokens, allowed_tokens=allowed_tokens, lm=lm, lm_weight=lm_weight, prefix_ids=prefix_ids)
        if gen.shape[1] < 2:                                  # labels need a target column
            gen = torch.nn.functional.pad(gen, (0, 2 - gen.shape[1]), value=c.pad_id)
        out = self.align(pixel_values, gen, layer=layer, top_k=top_k)
        ids = gen.cpu().numpy()
        tok = self.tokenizer
        alts = (out["alt_ids"].cpu().numpy(), out["alt_logprob"].cpu().numpy()) if top_k else None
        recs = A.build_records(ids, out["logprob"].cpu().numpy(), out["centroid"].cpu().numpy(), out["peak_patch"].cpu().numpy(),
                               pad_id=c.pad_id, bos_id=c.bos_id, eos_id=c.eos_id,
                               texts=None if tok is None else tok.batch_decode(gen, skip_special_tokens=True),
                               to_strings=None if tok is None else tok.convert_ids_to_tokens, alternatives=alts, forced=forced)
        if hyps is not None:
            for r, h in zip(recs, hyps):
                r["score"], r["hypotheses"] = h["score"], h["hypotheses"]
        return recs

    @contextlib.contextmanager
    def _decode_stream(self, use_graph: bool):
        """The stream a decode loop runs on, as ``(graph, keep)``.  ``graph``: the step is replayed from a hipGraph (``use_graph`` unless
        KZV_DECODE_GRAPH=0); stream capture needs a non-default stream, so the whole loop then runs on a side stream that starts
        behind the current one.  The body appends every tensor its kernels touched to ``keep``; on a clean exit the current stream
        waits for the side stream and the tensors are recorded on it.  After an exception neither happens."""
        import torch
        graph = use_graph and os.environ.get("KZV_DECODE_GRAPH", "1") != "0"
        cur = torch.cuda.current_stream(self.device)
        side = torch.cuda.Stream(self.device) if graph else cur
        if graph:
            side.wait_stream(cur)
        keep: list = []
        with torch.cuda.stream(side):
            yield graph, keep
        if graph:
            cur.wait_stream(side)
            for t_ in keep:
                t_.record_stream(cur)

    def generate(self, pixel_values, max_length: int = 128, num_beams: int = 1, early_stopping: bool = True,
                 length_penalty: float = 1.0, use_cache: bool = True, return_scores: bool = False,
                 no_repeat_ngram_size: int = 0, repetition_penalty: float = 1.0, min_length: int = 0, suppress_tokens=None, allowed_tokens=None,
                 lm=None, lm_weight: float = 0.0, num_return_sequences: int = 1, return_logprobs: bool = False, prefix_ids=None):
        """Decode from BOS.  The encoder (and the cross-attention K/V of every decoder layer) runs ONCE.
        ``num_return_sequences`` n in 1..num_beams / ``return_logprobs`` (the device hooks, as ``return_scores``; kzv/nbest.py): with
        n > 1 the ids are [B * n, W], HF's layout (image-major, best first) -- rows 0 .. n - 1 of every image's finished list, read off
        the search's own state -- and ``return_scores`` gives [B * n]; ``return_logprobs`` adds fp32 [B * n, W]: column t holds the
        log-probability of the token in column t, 0 in column 0 and from the row's length on (the search's own fp32 difference of
        accumulated scores: HF ``compute_transition_scores``; under controls or fusion the processed / fused row's value).  The results
        come in the order ids, scores, log-probabilities.
        ``return_scores`` (beam search on the device hooks only, i.e. 2..8 beams on the GPU): returns ``(ids, scores)``, scores fp32 [B] =
        the winners' sum of log-probabilities / generated length ** length_penalty (HF's ``sequences_scores``), read off the search's own
        state -- under generation controls the sum of the PROCESSED log-probabilities, which a teacher-forced pass cannot give.
        use_cache=True (default): each step feeds the newest token through the decoder against cached self-attention keys
        and values (kzv_decode_step); beam steps re-order the cache rows (kzv_decode_reorder).
        use_cache=False: each step is a decoder-only teacher-forced pass over the whole prefix (kzv_decode_logits), whose
        position-t logits only depend on ids[:, :t+1] under the causal mask -- the exact cross-check of the cached path.

        Token selection (greedy for num_beams == 1, else beam search with HF's rules) is kzv/beam.py, pinned on the CPU
        against transformers' own ``generate``; the reference asks for ``num_beams=4, early_stopping=True``
        (trocr_model.py:306-316).  The step logits come from this engine.

        Generation controls, with ``transformers.generate``'s names and semantics (kzv/controls.py; every default is off, and with all
        of them off nothing is launched for them): ``no_repeat_ngram_size`` g in 1..8 (no g-gram occurs twice), ``repetition_penalty``
        p > 0 (the scores of tokens already emitted are divided by p, or multiplied where negative), ``min_length`` (no EOS before the
        line holds that many tokens, BOS included; ``max_length`` still ends it), ``suppress_tokens`` (ids never chosen) or its
        complement ``allowed_tokens`` (EOS is always kept).  They act on every step's scores on the device (kzv_logits_process): on the
        raw logits for greedy decoding, on log_softmax(logits) before the beam score is added for beam search, as HF does.

        ``lm`` (a kzv.lm.NGramLM or its device form) with ``lm_weight`` != 0: shallow fusion of a character n-gram language model, every
        step's scores + lm_weight * log p_lm(token | the last order - 1 tokens), on the device (kzv_lm_fuse) AFTER the controls: greedy
        decoding takes arg-max of the fused logits; beam search adds it to the (processed) log-probabilities before the beam score and
        does not normalise again (kzv/lm.py states the rule).  ``lm=None`` or ``lm_weight=0``: off, nothing is built or launched.

        ``prefix_ids`` (a list of B id sequences, or a [B, P] tensor padded with pad_id; kzv/prefix.py): continue every line from given
        tokens -- HF's ``generate(input_ids=[BOS] + prefix)``, with lengths that may differ inside the batch.  The prefix holds no BOS /
        EOS / padding and 1 + len(prefix) <= max_length - 1, or the call refuses before any launch.  Every output row holds [BOS] +
        prefix + the generated tokens.  One decoder step per forced token (no prefill pass): while the chosen index lies inside an
        image's prefix its scores become -inf with 0 at the forced token (kzv_force_prefix), AFTER the controls and the language model,
        which do not act on the prompt but read it as history; ``max_length`` and ``min_length`` count it.  Beam scores sum the
        generated tokens only, and the length normalisation and the early-stop heuristic use the generated length.  A beam search
        with prefixes takes the normalise -> (fuse) -> force -> rank-log-probabilities route.  None or all empty: off, nothing is
        launched."""
        import torch
        from . import beam as BM
        from . import prefix as PF
        from . import controls as CT
        from . import lm as LM
        c = self.cfg
        ctl = CT.from_kwargs(c.eos_id, no_repeat_ngram_size, repetition_penalty, min_length, suppress_tokens, allowed_tokens)
        lmr = LM.resolve(lm, lm_weight, c.vocab, self.device)          # (host model, device tables, weight) or None
        ctl_mask = None
        if ctl is not None:
            ctl.check(c.vocab, c.eos_id, num_beams)
            ctl_mask = ctl.mask(c.vocab, c.eos_id)
            ctl_mask = None if ctl_mask is None else ctl_mask.to(self.device)
        px = self._check_inputs(pixel_values)
        B = px.shape[0]
        Lh = min(max_length, c.max_pos - c.pad_id - 1)
        pfx = PF.resolve(prefix_ids, B, c, Lh, self.device)            # the tables on the device, or None: off (refusals before any launch)
        lib = L.load()
        was = self.training
        self.training = False
        nb = max(1, int(num_beams))
        if return_scores and nb == 1:
            raise ValueError("return_scores needs num_beams > 1")
        from . import nbest as NB
        n_ret = NB.check_request(nb, num_return_sequences, return_logprobs, "generate")
        if return_logprobs and nb == 1:
            raise ValueError("generate: return_logprobs needs num_beams > 1 (greedy decoding returns them from generate_stream)")
        nbest = n_ret > 1 or bool(return_logprobs)
        BB = B * nb
        # cached decoding runs the encoder and the cross-attention K/V once per IMAGE (kzv_encode_images): beams share them, and no
        # teacher-forced decoder pass is spent on the BOS-only prompt
        share = use_cache
        if nb > 1 and not share:
            px = px.repeat_interleave(nb, dim=0)
        ids0 = torch.full((BB, Lh), c.pad_id, dtype=torch.int64, device=self.device)
        ids0[:, 0] = c.bos_id
        step_logits = torch.empty(BB, c.vocab, dtype=torch.float32, device=self.device)
        if share:
            self._bind(BB, Lh)
            self._keep = (px, ids0)
            L.check(lib.kzv_encode_images(self._h, px.data_ptr(), B, L.stream_handle()), "encode_images")
        else:
            self.forward_loss(px, ids0, want_logits=False, seed=0)          # encoder + cross K/V (and a first decoder pass)
        state = {"valid": torch.zeros(BB, Lh, dtype=torch.uint8, device=self.device)}   # self-attention keys usable (token != pad)
        posids = torch.empty(BB, dtype=torch.int32, device=self.device)
        tok_buf = torch.empty(BB, dtype=torch.int64, device=self.device)
        # the cached step is ~100 small launches: replayed from a hipGraph (kzv_decode_step_graph) where _decode_stream says so (`graph`,
        # bound by the `with` below before any step runs)
        self.last_generate_steps = 0             # decoder steps this call issued (those run past the end before the host looked included)

        def step(t, ids):
            self.last_generate_steps += 1
            if not use_cache:
                ids = ids.contiguous()
                state["ids"] = ids                                        # keep alive until the kernels have run
                L.check(lib.kzv_set_active_length(self._h, t + 1), "set_active_length")   # later positions are not needed
                L.check(lib.kzv_decode_logits(self._h, ids.data_ptr(), t, step_logits.data_ptr(), L.stream_handle()), "decode_logits")
                return step_logits
            valid = state["valid"]
            # newest token, RoBERTa position id (modeling_roberta.py:142-155: cumsum of non-pad tokens + pad_id; prefixes never
            # hold pads) and the key-usable flag of column t, in one launch
            L.check(lib.kzv_decode_prep(ids.data_ptr(), ids.stride(0), t, c.pad_id, BB, tok_buf.data_ptr(), valid.data_ptr(), Lh,
                                        posids.data_ptr(), L.stream_handle()), "decode_prep")
            if graph:
                L.check(lib.kzv_decode_step_graph(self._h, tok_buf.data_ptr(), posids.data_ptr(), valid.data_ptr(), Lh, step_logits.data_ptr(),
                                                  L.stream_handle()), "decode_step_graph")
            else:
                L.check(lib.kzv_decode_step(self._h, tok_buf.data_ptr(), posids.data_ptr(), t, valid.data_ptr(), Lh, step_logits.data_ptr(),
                                            L.stream_handle()), "decode_step")
            return step_logits

        def reorder(rows, n_keys):
            if use_cache:
                rows = rows.contiguous()
                state["valid"].copy_(state["valid"][rows])                # in place: the graph holds this buffer's address
                L.check(lib.kzv_decode_reorder(self._h, rows.data_ptr(), n_keys, L.stream_handle()), "decode_reorder")

        def controls_hook(scores, ids, n, normalise=0):
            """The controls on ``scores`` [BB, V] in place, histories ids[:, :n] (kzv_logits_process; ``controls_impl`` = "reference"
            substitutes the torch statement on the same scores: the whole-decode tests compare the two)."""
            if self.controls_impl == "reference" and ctl is not None:
                x = torch.log_softmax(scores, dim=-1) if normalise else scores
                scores.copy_(CT.process_reference(x, ids[:, :n], ctl, c.eos_id))
                return scores
            if scores.stride(1) != 1 or ids.stride(1) != 1:
                raise ValueError("controls: scores and ids must be dense along their rows")
            k = ctl if ctl is not None else neutral      # the language model alone in a beam search: the kernel only normalises
            a = L.kzv_logits_process_args(logits=scores.data_ptr(), ld=scores.stride(0), rows=scores.shape[0], vocab=c.vocab, ids=ids.data_ptr(),
                                          ld_ids=ids.stride(0), t=n - 1, group=1, slot_image=None, slot_t=None, by_image=0, n_images=0,
                                          no_repeat_ngram_size=k.no_repeat_ngram_size, min_length=k.min_length, eos_id=c.eos_id,
                                          normalise=1 if normalise else 0, repetition_penalty=k.repetition_penalty, reserved=0,
                                          suppress_mask=L.ptr(ctl_mask))
            L.check(lib.kzv_logits_process(C.byref(a), L.stream_handle()), "logits_process")
            return scores

        def lm_hook(scores, ids, n):
            """+ lm_weight * lm on ``scores`` [BB, V] in place, histories ids[:, :n] (kzv_lm_fuse; ``lm_impl`` = "reference" substitutes
            kzv/lm.py::fuse_reference on the same scores)."""
            host, dlm, w = lmr
            if self.lm_impl == "reference":
                scores.copy_(LM.fuse_reference(scores, ids[:, :n], host, w))
                return scores
            if scores.stride(1) != 1 or ids.stride(1) != 1:
                raise ValueError("lm: scores and ids must be dense along their rows")
            a = L.kzv_lm_fuse_args(logits=scores.data_ptr(), ld=scores.stride(0), rows=scores.shape[0], vocab=c.vocab, ids=ids.data_ptr(),
                                   ld_ids=ids.stride(0), t=n - 1, group=1, slot_image=None, slot_t=None, by_image=0, n_images=0, weight=w,
                                   reserved=0, lm=C.pointer(dlm.struct))
            L.check(lib.kzv_lm_fuse(C.byref(a), L.stream_handle()), "lm_fuse")
            return scores

        def prefix_hook(scores, ids, n, normalised=0):
            """The forced prefixes on ``scores`` [BB, V] in place, nb rows per image, the token chosen being column n (kzv_force_prefix;
            ``prefix_impl`` = "reference" substitutes kzv/prefix.py::force_reference on the same scores)."""
            if self.prefix_impl == "reference":
                scores.copy_(PF.force_reference(scores, n, *pfx.rows(nb)))
                return scores
            if scores.stride(1) != 1:
                raise ValueError("prefix: scores must be dense along their rows")
            a = L.kzv_force_prefix_args(logits=scores.data_ptr(), ld=scores.stride(0), rows=scores.shape[0], vocab=c.vocab, t=n - 1, group=nb,
                                        slot_image=None, slot_t=None, by_image=0, n_images=B, prefix=pfx.prefix.data_ptr(), ld_prefix=pfx.width,
                                        prefix_len=pfx.prefix_len.data_ptr(), normalised=1 if normalised else 0, reserved=0,
                                        forced_logprob=None, ld_forced_logprob=0)
            L.check(lib.kzv_force_prefix(C.byref(a), L.stream_handle()), "force_prefix")
            return scores

        def chain_hook(scores, ids, n):          # the one order everywhere: controls first, then the language model, then the prefix
            if ctl is not None:
                scores = controls_hook(scores, ids, n)
            if lmr:
                scores = lm_hook(scores, ids, n)
            return prefix_hook(scores, ids, n) if pfx is not None else scores

        neutral = CT.GenerationControls()
        topk = update = None
        process = chain_hook if (ctl is not None or lmr or pfx is not None) else None
        raw_step = step

        def step_logprobs(t, ids):               # beams on the device ranking: normalise + process here, rank log-probabilities after
            x = controls_hook(raw_step(t, ids), ids, t + 1, normalise=1)
            x = lm_hook(x, ids, t + 1) if lmr else x
            return prefix_hook(x, ids, t + 1, normalised=1) if pfx is not None else x

        def torch_beam_hook(scores, ids, n):     # the torch ranking forces the rows itself (beam_search's ``prefix``): controls and the language model only
            if ctl is not None:
                scores = controls_hook(scores, ids, n)
            return lm_hook(scores, ids, n) if lmr else scores

        bprefix = None if pfx is None else (pfx.prefix, pfx.prefix_len)

        try:
            with self._decode_stream(use_cache) as (graph, keep):
                # the hooks allocate and zero their flag / top-k buffers: on the stream whose kernels read them
                if nb > 1 and nb <= 8 and self.device.type == "cuda" and os.environ.get("KZV_BEAM_TOPK", "1") != "0":
                    topk, update = BM.make_device_hooks(B, nb, Lh, c.vocab, c.eos_id, early_stopping, length_penalty, self.device,
                                                        logprobs=ctl is not None or lmr is not None or pfx is not None,
                                                        prefix_len=None if pfx is None else pfx.prefix_len)
                    if os.environ.get("KZV_BEAM_UPDATE", "1") == "0":
                        update = None
                    if ctl is not None or lmr is not None or pfx is not None:
                        step, process = step_logprobs, None
                if nb > 1 and process is not None:
                    process = torch_beam_hook if (ctl is not None or lmr) else None
                if use_cache:
                    L.check(lib.kzv_set_active_length(self._h, 1), "set_active_length")
                    L.check(lib.kzv_decode_begin(self._h, L.stream_handle()), "decode_begin")
                if nb == 1:
                    gupd = BM.make_greedy_hook(B, c.vocab, c.pad_id, c.eos_id, self.device, Lh) if self.device.type == "cuda" and os.environ.get("KZV_BEAM_TOPK", "1") != "0" else None
                    out = BM.greedy(step, B, Lh, c.pad_id, c.bos_id, c.eos_id, self.device, update=gupd, process=process)
                elif nbest:                                       # rows 0 .. n - 1 of the finished lists, off the search's own state
                    if topk is None or update is None:
                        raise ValueError("num_return_sequences / return_logprobs need the device beam hooks (2..8 beams on the GPU, KZV_BEAM_TOPK / KZV_BEAM_UPDATE on)")
                    res, bst = BM.beam_search_fused(step, reorder, B, nb, Lh, c.vocab, c.pad_id, c.bos_id, c.eos_id, self.device, early_stopping,
                                                    length_penalty, topk, update, return_state=True, num_return_sequences=n_ret,
                                                    return_logprobs=bool(return_logprobs))
                    NB.check_done(res["lengths"], "generate")
                    self.last_generate_lengths = res["lengths"]      # tokens per returned row, BOS included (a row may END in padding at max_length)
                    out, scores, lps = res["ids"], res["scores"], res.get("logprobs")
                    keep += [t for t in (scores, lps) if t is not None]
                elif return_scores:                               # (what beam_search runs with both hooks; the state holds the scores)
                    if topk is None or update is None:
                        raise ValueError("return_scores needs the device beam hooks (2..8 beams on the GPU, KZV_BEAM_TOPK / KZV_BEAM_UPDATE on)")
                    out, bst = BM.beam_search_fused(step, reorder, B, nb, Lh, c.vocab, c.pad_id, c.bos_id, c.eos_id, self.device, early_stopping,
                                                    length_penalty, topk, update, return_state=True)
                    scores = bst["fin_sc"][:, 0].clone()
                else:
                    out = BM.beam_search(step, reorder, B, nb, Lh, c.vocab, c.pad_id, c.bos_id, c.eos_id, self.device,
                                         early_stopping=early_stopping, length_penalty=length_penalty, topk=topk, update=update,
                                         process=process, prefix=bprefix)
                keep += (out, step_logits, posids, tok_buf, state["valid"], px) + (() if ctl_mask is None else (ctl_mask,))
                if lmr:
                    keep += lmr[1].keep()
                if pfx is not None:
                    keep += pfx.keep()
                if return_scores:
                    keep.append(scores)
            if nbest:
                got = (out,) + ((scores,) if return_scores else ()) + ((lps,) if return_logprobs else ())
                return got if len(got) > 1 else out
            return (out, scores) if return_scores else out
        finally:
            self.training = was

    # ------------------------------------------------------------------ greedy decoding of many images (slot refill)
    @property
    def stream_decode_impl(self) -> str:
        """"slot-refill" | "static": what ``generate_stream`` on this model runs (kzv_stream_decode_impl: the bound decoder geometry,
        the crop width of the last call, the kzv_set_decode_one_launch mode).  "static" is lockstep ``generate(num_beams=1)`` over
        batches of ``slots``: the same results without the saving.  Valid once a generate / generate_stream (or _bind) has bound the
        model."""
        rc = L.load().kzv_stream_decode_impl(self._h)
        if rc < 0:
            L.check(rc, "kzv_stream_decode_impl")
        return "slot-refill" if rc == 1 else "static"

    def stream_beam_impl_for(self, num_beams: int) -> str:
        """"slot-refill" | "static": what ``generate_stream(num_beams=num_beams)`` on this model runs (kzv_stream_beam_impl: 2 or 4 beams,
        the bound rows a multiple of them, and stream_decode_impl's conditions for that many rows per image).  "static" is lockstep
        ``generate(num_beams=num_beams)`` over batches of ``slots``."""
        rc = L.load().kzv_stream_beam_impl(self._h, int(num_beams))
        if rc < 0:
            L.check(rc, "kzv_stream_beam_impl")
        return "slot-refill" if rc == 1 else "static"

    @property
    def stream_beam_impl(self) -> str:
        """``stream_beam_impl_for`` the beam count of the last ``generate_stream(num_beams > 1)`` call (4 before any)."""
        return self.stream_beam_impl_for(self._stream_beams)

    @staticmethod
    def _waves(pixel_values, wave: int):
        """[N, C, H, W] or an iterable of such batches -> tensors of exactly ``wave`` images (the last one shorter)."""
        import torch
        if torch.is_tensor(pixel_values):
            pixel_values = (pixel_values,)
        held, n = [], 0
        for b in pixel_values:
            held.append(b); n += b.shape[0]
            while n >= wave:
                allb = torch.cat(held) if len(held) > 1 else held[0]
                yield allb[:wave]
                held, n = ([allb[wave:]], allb.shape[0] - wave) if allb.shape[0] > wave else ([], 0)
        if n:
            yield torch.cat(held) if len(held) > 1 else held[0]

    def generate_stream(self, pixel_values, max_length: int = 128, slots: int | None = None, limits=None, return_logprobs: bool = False,
                        pool_bytes: int = 4 << 30, num_beams: int = 1, early_stopping: bool = True, length_penalty: float = 1.0,
                        return_scores: bool = False, top_k: int = 0,
                        no_repeat_ngram_size: int = 0, repetition_penalty: float = 1.0, min_length: int = 0, suppress_tokens=None, allowed_tokens=None,
                        lm=None, lm_weight: float = 0.0, num_return_sequences: int | None = None, prefix_ids=None,
                        return_prefix_logprobs: bool = False):
        """Greedy decoding of N images, N much larger than a batch, over a fixed set of ``slots`` decoder rows that the DEVICE keeps
        full: a slot whose line has ended takes the next waiting image and restarts at BOS in the very next step (kzv/stream.py states
        the bookkeeping; include/kzv.h: kzv_stream_*), where ``generate`` would run every batch until its longest line has ended.

        ``pixel_values``: [N, C, H, W] on host or device, or an iterable of such batches (one crop width).  ``slots`` defaults to the
        device's compute-unit count (one workgroup of the one-launch step fills a CU).  ``limits``: optional [N] ints, the most tokens,
        BOS included, each image may get (a bound for junk crops that would otherwise run to max_length).  The images are taken in
        WAVES as large as ``pool_bytes`` allows (dec_layers * 2 * patches * dec_hidden * 2 bytes of cross-attention K/V per image):
        a wave is encoded first, then decoded.  Returns int64 [N, <= max_length] in input order -- BOS, the tokens, EOS if emitted,
        padding -- and with ``return_logprobs`` also fp32 of the same shape, the log-probability of every emitted token at its column.
        Without ``limits`` each row equals the matching row of ``generate(num_beams=1)``; with them, that row cut at the limit.
        Where ``stream_decode_impl`` says "static" this IS ``generate(num_beams=1)`` over batches of ``slots`` (log-probabilities then
        from ``align``).

        ``num_beams`` > 1: beam search with ``generate``'s rules (``early_stopping``, ``length_penalty``) -- what the reference asks for
        on every validation and test image.  With 2 or 4 beams a slot holds an image's whole beam group (``slots * num_beams`` decoder
        rows are bound) and takes the next image the step after its search has ended (kzv/stream.py: beam_stream); every row equals
        the matching row of ``generate(num_beams=num_beams)``, with ``limits`` that of ``generate(max_length=limit)``.  Other beam
        counts, or ``stream_beam_impl_for(num_beams) == "static"``, run ``generate`` over batches of ``slots``: the same rows.
        ``return_scores``: also fp32 [N], the winner's sum of log-probabilities / generated length ** length_penalty (HF's
        ``sequences_scores``; on the static path from ``align``).  ``return_logprobs`` with beams needs ``num_return_sequences`` stated
        (below); without it the call refuses, as it did.  The slots assume that no running beam holds padding; a wave in which one took ``pad_id`` is
        decoded again by ``generate`` and counted in ``last_stream_pad_fallbacks``.

        ``top_k`` in 1..8 (greedy only): the call returns ``(ids, logprobs, alt_ids, alt_logprob)``, the last two int64 / fp32
        [N, width, top_k]: at every emitted column the k best tokens of that step and their log-probabilities, best first (entry 0 is
        the emitted token; kzv_stream_topk, one more kernel per step and no second pass); -1 / 0 in column 0 and past a line's end.  On
        the static path they come from ``align(..., top_k=top_k)``.

        Generation controls (``generate``'s five keywords, same semantics; defaults off): every step of a wave runs kzv_logits_process as
        one more node of its captured chain (kzv_stream_set_controls), on each slot's own history; a beam wave normalises, processes and
        ranks without normalising again.  Every row still equals the matching row of ``generate`` called with the same controls, and
        the two fallbacks -- "static" geometries and a beam wave decoded again after a padding continuation -- carry them too.  With
        controls on, ``return_logprobs`` and the ``top_k`` alternatives are those of the PROCESSED row (HF's
        ``scores[t].log_softmax(-1)``): a banned token never appears among the alternatives (it ranks last at -inf).  On the static path
        the log-probabilities stay the model's own (``align``).  Tip: ``suppress_tokens=[pad_id]`` removes the cause of the beam
        stream's re-decode -- no running beam can take padding.

        Language-model fusion (``lm``, ``lm_weight``: ``generate``'s keywords and rule; off by default): every step of a wave runs
        kzv_lm_fuse as one more node of its captured chain, after the controls' node (kzv_stream_set_lm), on each slot's own history; a
        beam wave then normalises through the controls' kernel even when the controls are neutral.  Every row still equals the matching
        row of ``generate`` called with the same keywords, both fallbacks carry them, and ``return_logprobs`` / ``top_k`` are those of
        the FUSED row.

        ``num_return_sequences`` n in 1..num_beams (beams only; kzv/nbest.py): the n best readings of every line, ids [N * n, width] in
        HF's layout (image-major, best first; rows 0::n are the rows without it), ``return_scores`` then fp32 [N * n]; stating it --
        ``num_return_sequences=1`` serves a winner -- also admits ``return_logprobs`` for a beam search: fp32 [N * n, width], column
        t the log-probability of the token in column t, 0 in column 0 and from the row's length on, the search's own values
        (kzv_stream_set_nbest; one more staged row copy per step).  The results come in the order ids, scores, log-probabilities.  Both
        fallbacks call ``generate`` with the same keywords and return the same rows.

        Forced prefixes (``prefix_ids``: ``generate``'s keyword and rule, one entry per image of the whole call; off by default): every
        step of a wave runs kzv_force_prefix as the LAST node of its captured chain before selection (kzv_stream_set_prefix), on each
        slot's own image and step, so a slot that is reseated in the middle of another image's prefix reads its new image's from step 0;
        a beam wave takes the rank-log-probabilities route and its update the images' own generated lengths.  ``limits`` count the
        prefix (1 + len(prefix) <= limit - 1).  Every row still equals the matching row of ``generate(prefix_ids=...)``; both fallbacks
        pass the prefixes on; ``return_logprobs`` holds exactly 0 at forced columns.  ``return_prefix_logprobs``: one more result at the
        end, fp32 [N, width]: at every forced column the MODEL's log-probability of the forced token -- taken off the row before it is
        overwritten, after controls and fusion -- and 0 elsewhere (slot-refill waves only; refused on the fallbacks' geometries)."""
        import torch
        from . import controls as CT
        from . import lm as LM
        from . import nbest as NB
        from . import prefix as PF
        c = self.cfg
        n_ret = NB.check_request(num_beams, 1 if num_return_sequences is None else num_return_sequences, return_logprobs, "generate_stream")
        nbest = n_ret if num_return_sequences is not None and int(num_beams) > 1 and (n_ret > 1 or return_logprobs) else 0
        ctl = CT.from_kwargs(c.eos_id, no_repeat_ngram_size, repetition_penalty, min_length, suppress_tokens, allowed_tokens)
        lmr = LM.resolve(lm, lm_weight, c.vocab, self.device)          # before any wave runs; None: off
        if ctl is not None:
            ctl.check(c.vocab, c.eos_id, num_beams)   # before any wave runs
        nb = int(num_beams)
        top_k = int(top_k)
        if nb < 1:
            raise ValueError("num_beams must be positive")
        if not 0 <= top_k <= 8:
            raise ValueError("top_k must be in 0..8")
        if nb > 1 and top_k:
            raise ValueError("top_k is greedy only: a beam winner's per-token candidates are not produced on the slots (recognize(top_k=...) scores them in a teacher-forced pass)")
        if top_k:
            return_logprobs = True
        if nb > 1 and return_logprobs and not nbest:
            raise ValueError("return_logprobs is greedy only: a beam search returns sequence scores (return_scores), and its per-token "
                             "log-probabilities where num_return_sequences is stated")
        if nb == 1 and return_scores:
            raise ValueError("return_scores needs num_beams > 1 (greedy decoding returns per-token log-probabilities: return_logprobs)")
        beams = None if nb == 1 else (nb, bool(early_stopping), float(length_penalty))
        if beams:
            self._stream_beams = nb
        self.last_stream_pad_fallbacks = 0       # running beams that took padding in the waves decoded again by generate
        Lh = min(max_length, c.max_pos - c.pad_id - 1)
        if Lh < 2:
            raise ValueError("max_length must be at least 2")
        if slots is None:
            slots = torch.cuda.get_device_properties(self.device).multi_processor_count
        slots = int(slots)
        if slots < 1:
            raise ValueError("slots must be positive")
        lim_all = None if limits is None else torch.as_tensor(limits, dtype=torch.int32).reshape(-1).clamp(min=2)
        pfx_all = None                            # the whole call's prefixes, checked before any wave runs; None: off
        if prefix_ids is not None:
            n_pfx = prefix_ids.n if isinstance(prefix_ids, PF.Prefixes) else len(prefix_ids)
            if lim_all is not None and lim_all.numel() != n_pfx:
                raise ValueError("limits and prefix_ids must both hold one entry per image")
            pfx_all = PF.resolve(prefix_ids, n_pfx, c, Lh, self.device, limits=lim_all)
        if return_prefix_logprobs and pfx_all is None:
            raise ValueError("return_prefix_logprobs needs prefix_ids with at least one forced token")
        if return_prefix_logprobs and nbest:
            raise ValueError("return_prefix_logprobs is not combined with num_return_sequences")
        pl_out = []
        ids_out, lp_out, alt_out, nb_out, done = [], [], [], [], 0
        self.last_stream_steps = 0               # decoder steps the last call took (every wave; the static path leaves 0)
        src = iter((pixel_values,) if torch.is_tensor(pixel_values) else pixel_values)
        first_batch = next(src)
        src = itertools.chain((first_batch,), src)
        per_image = c.dec_layers * 2 * (c.image_h // c.patch_h) * (first_batch.shape[3] // c.patch_w) * c.dec_hidden * 2
        wave = max(slots, int(pool_bytes) // per_image // slots * slots)
        for px in self._waves(src, wave):
            n = px.shape[0]
            lim = None if lim_all is None else lim_all[done:done + n]
            if lim is not None and lim.numel() != n:
                raise ValueError("limits must hold one entry per image")
            pfx = None
            if pfx_all is not None:               # the wave's own tables (None when all of its prefixes are empty: the wave runs as today)
                if done + n > pfx_all.n:
                    raise ValueError("prefix_ids must hold one entry per image")
                pfx = pfx_all.slice(done, done + n, want_logprobs=bool(return_prefix_logprobs))
            if return_prefix_logprobs:
                self._wave_forced_lp = None
            if nbest:
                nb_out.append(self._stream_wave(px, Lh, slots, lim, bool(return_logprobs), beams, 0, ctl, lmr, nbest, pfx))
                done += n
                continue
            if top_k:
                ids, lp, alts = self._stream_wave(px, Lh, slots, lim, return_logprobs, beams, top_k, ctl, lmr, 0, pfx)
                alt_out.append(alts)
            else:
                ids, lp = self._stream_wave(px, Lh, slots, lim, return_logprobs, beams, 0, ctl, lmr, 0, pfx)
            if return_prefix_logprobs:
                fl = torch.zeros(n, Lh, dtype=torch.float32, device=self.device)
                if pfx is not None:
                    if self._wave_forced_lp is None:
                        raise ValueError("return_prefix_logprobs: this wave ran on lockstep generate (a geometry without slot-refill decoding, or "
                                         "a beam wave decoded again), which does not record them")
                    fl[:, :pfx.width + 1] = self._wave_forced_lp
                pl_out.append(fl)
            ids_out.append(ids); lp_out.append(lp); done += n
        if pfx_all is not None and done != pfx_all.n:
            raise ValueError(f"prefix_ids holds {pfx_all.n} prefixes for {done} images")
        if nbest:                                 # waves concatenate image-major
            lengths = torch.cat([w["lengths"] for w in nb_out])
            NB.check_done(lengths, "generate_stream")
            width = max(2, int(lengths.max()))
            got = (torch.cat([w["ids"] for w in nb_out])[:, :width],)
            got += (torch.cat([w["scores"] for w in nb_out]),) if return_scores else ()
            got += (torch.cat([w["logprobs"] for w in nb_out])[:, :width],) if return_logprobs else ()
            return got if len(got) > 1 else got[0]
        ids = torch.cat(ids_out)
        width = max(2, int((ids != c.pad_id).sum(dim=1).max()))
        tail = (torch.cat(pl_out)[:, :width],) if return_prefix_logprobs else ()
        if top_k:
            return (ids[:, :width], torch.cat(lp_out)[:, :width], torch.cat([a[0] for a in alt_out])[:, :width].long(),
                    torch.cat([a[1] for a in alt_out])[:, :width]) + tail
        if return_logprobs:
            return (ids[:, :width], torch.cat(lp_out)[:, :width]) + tail
        if return_scores:
            return (ids[:, :width], torch.cat(lp_out)) + tail
        return (ids[:, :width],) + tail if tail else ids[:, :width]

    @staticmethod
    def _controls_kw(ctl, lmr=None) -> dict:
        """``generate``'s keywords for the controls and the language model of a wave (none when they are off)."""
        kw = {} if lmr is None else {"lm": lmr[1], "lm_weight": lmr[2]}
        if ctl is None:
            return kw
        return dict(kw, no_repeat_ngram_size=ctl.no_repeat_ngram_size, repetition_penalty=ctl.repetition_penalty, min_length=ctl.min_length,
                    suppress_tokens=ctl.suppress_tokens, allowed_tokens=ctl.allowed_tokens)

    def _static_beam_wave(self, px, Lh: int, slots: int, lim, beams, ctl=None, lmr=None, pfx=None):
        """``generate(num_beams=nb)`` over batches of ``slots``: ids [n, Lh] and the winners' scores [n] (from a teacher-forced pass).  With
        limits, the images of every distinct limit are decoded with it as their max_length.  ``pfx``: the wave's forced prefixes
        (kzv/prefix.py: Prefixes) or None; they go to ``generate`` with their images, and the score sums the generated tokens only."""
        import torch
        c = self.cfg
        nb, early, lpen = beams
        n, dev = px.shape[0], self.device
        ids = torch.full((n, Lh), c.pad_id, dtype=torch.int64, device=dev)
        score = torch.zeros(n, dtype=torch.float32, device=dev)
        lim = None if lim is None else lim.cpu().clamp(max=Lh)
        groups = [(Lh, torch.arange(n))] if lim is None else [(int(v), (lim == v).nonzero().reshape(-1)) for v in lim.unique().tolist()]
        for width, idx in groups:
            for a in range(0, idx.numel(), slots):
                sel = idx[a:a + slots]
                sub = px[sel.to(px.device)]
                sub_pfx = None if pfx is None else pfx.select(sel)
                g = self.generate(sub, max_length=width, num_beams=nb, early_stopping=early, length_penalty=lpen, prefix_ids=sub_pfx,
                                  **self._controls_kw(ctl, lmr))
                rows = torch.full((sel.numel(), Lh), c.pad_id, dtype=torch.int64, device=dev)
                rows[:, :g.shape[1]] = g
                sc = self.align(sub, rows)
                live = sc["live"].float()
                if sub_pfx is not None:               # row t of align belongs to column t + 1: the forced columns 1 .. len do not count
                    live = live * (torch.arange(live.shape[1], device=dev).view(1, -1) >= sub_pfx.prefix_len.view(-1, 1)).float()
                ids[sel.to(dev)] = rows
                score[sel.to(dev)] = (sc["logprob"] * live).sum(1) / live.sum(1).clamp(min=1).pow(lpen)
        return ids, score

    def _stream_wave(self, px, Lh: int, slots: int, lim, want_lp: bool, beams=None, top_k: int = 0, ctl=None, lmr=None, nbest: int = 0, pfx=None):
        """One wave of generate_stream: ids [n, Lh] and log-probabilities [n, Lh] or None; with ``beams`` = (num_beams, early_stopping,
        length_penalty): ids [n, Lh] and the winners' scores [n]; with ``top_k`` (greedy) a third result, (alt_ids int32, alt_logprob)
        [n, Lh, top_k].  ``ctl``: the wave's GenerationControls (None: off); ``lmr``: its language model (kzv/lm.py: resolve; None: off).
        ``nbest`` n >= 1 (beams): the result is kzv/nbest.py's dict of the n best rows per image instead (``want_lp``: with log-probabilities).
        ``pfx``: the wave's forced prefixes (kzv/prefix.py: Prefixes; None: off), indexed by the wave's images; where it holds a
        forced_logprob table, a slot-refill wave leaves it in ``self._wave_forced_lp``."""
        import torch
        from . import nbest as NB
        from . import stream as ST
        c = self.cfg
        lib = L.load()
        n = px.shape[0]
        dev = self.device
        self._check_inputs(px[:1])                                # geometry checks + the active crop width
        nb = beams[0] if beams else 1
        static_beams = (lambda px_, Lh_, slots_, lim_, beams_, ctl_, lmr_: self._static_beam_wave(px_, Lh_, slots_, lim_, beams_, ctl_, lmr_, pfx)) if not nbest else (
            lambda px_, Lh_, slots_, lim_, beams_, ctl_, lmr_: NB.static_wave(self, px_, Lh_, slots_, lim_, beams_, nbest, want_lp, self._controls_kw(ctl_, lmr_),
                                                                              prefixes=pfx))
        if beams and nb not in (2, 4):
            return static_beams(px, Lh, slots, lim, beams, ctl, lmr)
        rows = slots * nb                                         # decoder rows: a slot holds one sequence, or an image's beam group
        self._bind(rows, Lh)
        if beams and self.stream_beam_impl_for(nb) == "static":
            return static_beams(px, Lh, slots, lim, beams, ctl, lmr)
        if not beams and self.stream_decode_impl == "static":
            ids = torch.full((n, Lh), c.pad_id, dtype=torch.int64, device=dev)
            lp = torch.zeros(n, Lh, dtype=torch.float32, device=dev) if want_lp else None
            alt_ids = torch.full((n, Lh, top_k), -1, dtype=torch.int32, device=dev) if top_k else None
            alt_lp = torch.zeros(n, Lh, top_k, dtype=torch.float32, device=dev) if top_k else None
            for a in range(0, n, slots):
                g = self.generate(px[a:a + slots], max_length=Lh, num_beams=1, prefix_ids=None if pfx is None else pfx.slice(a, a + slots),
                                  **self._controls_kw(ctl, lmr))
                ids[a:a + g.shape[0], :g.shape[1]] = g
            if lim is not None:
                ids = torch.where(torch.arange(Lh, device=dev).view(1, Lh) >= lim.to(dev).view(n, 1), torch.full_like(ids, c.pad_id), ids)
            if want_lp:
                for a in range(0, n, slots):
                    sc = self.align(px[a:a + slots], ids[a:a + slots], top_k=top_k)
                    lp[a:a + slots, 1:] = torch.where(sc["live"], sc["logprob"], torch.zeros_like(sc["logprob"]))
                    if top_k:
                        lv = sc["live"].unsqueeze(-1)
                        alt_ids[a:a + slots, 1:] = torch.where(lv, sc["alt_ids"], torch.full_like(sc["alt_ids"], -1)).to(torch.int32)
                        alt_lp[a:a + slots, 1:] = torch.where(lv, sc["alt_logprob"], torch.zeros_like(sc["alt_logprob"]))
            return (ids, lp, (alt_ids, alt_lp)) if top_k else (ids, lp)
        was = self.training
        self.training = False
        ids = torch.full((n, Lh), c.pad_id, dtype=torch.int64, device=dev)
        ids[:, 0] = c.bos_id
        lp = torch.zeros(n, Lh, dtype=torch.float32, device=dev) if want_lp and not nbest else None
        score = torch.zeros(n, dtype=torch.float32, device=dev) if beams else None
        nbo = NB.WaveOutputs(n, nbest, Lh, c.pad_id, c.bos_id, dev, want_lp) if nbest else None
        alt_ids = torch.full((n, Lh, top_k), -1, dtype=torch.int32, device=dev) if top_k else None
        alt_lp = torch.zeros(n, Lh, top_k, dtype=torch.float32, device=dev) if top_k else None
        limd = None if lim is None else lim.to(dev).contiguous()
        pool = -(-n // rows) * rows
        divisors = [d for d in range(1, rows + 1) if rows % d == 0]
        try:
            with self._decode_stream(True) as (graph, keep):
                st = L.stream_handle()
                if beams:
                    L.check(lib.kzv_stream_begin_beams(self._h, nb, 1 if beams[1] else 0, beams[2], score.data_ptr(), pool, n, Lh, c.bos_id, c.eos_id,
                                                       ids.data_ptr(), Lh, None, 0, L.ptr(limd), st), "stream_begin_beams")
                    if nbo is not None:
                        nbo.arm(lib, self._h, st, L.check)
                else:
                    L.check(lib.kzv_stream_begin(self._h, pool, n, Lh, c.bos_id, c.eos_id, ids.data_ptr(), Lh, L.ptr(lp), Lh, L.ptr(limd), st), "stream_begin")
                    if top_k:
                        L.check(lib.kzv_stream_set_topk(self._h, top_k, alt_ids.data_ptr(), alt_lp.data_ptr(), Lh * top_k, st), "stream_set_topk")
                if ctl is not None:                               # one more node per step; the library copies the (host) mask
                    mk = ctl.mask(c.vocab, c.eos_id)
                    cc = L.kzv_logits_controls(no_repeat_ngram_size=ctl.no_repeat_ngram_size, repetition_penalty=ctl.repetition_penalty,
                                               min_length=ctl.min_length, reserved=0, suppress_mask=None if mk is None else mk.data_ptr())
                    L.check(lib.kzv_stream_set_controls(self._h, C.byref(cc), st), "stream_set_controls")
                if lmr is not None:                               # and one more after it; the tables stay ours for the wave
                    L.check(lib.kzv_stream_set_lm(self._h, C.byref(lmr[1].struct), lmr[2], st), "stream_set_lm")
                    keep += lmr[1].keep()
                if pfx is not None:                               # the chain's last node before selection; the tables stay ours for the wave
                    L.check(lib.kzv_stream_set_prefix(self._h, pfx.prefix.data_ptr(), pfx.width, pfx.prefix_len.data_ptr(), L.ptr(pfx.forced_logprob),
                                                      pfx.width + 1, st), "stream_set_prefix")
                    keep += pfx.keep()
                a = 0
                while a < n:                                      # the encoder runs on divisors of the bound batch; a short last batch
                    k = min(rows, n - a)                          # is filled by repeating its last image
                    d = next(x for x in divisors if x >= k)
                    chunk = px[a:a + k].to(dev, dtype=torch.float32)
                    if d > k:
                        chunk = torch.cat((chunk, chunk[-1:].expand(d - k, -1, -1, -1)))
                    chunk = chunk.contiguous()
                    keep.append(chunk)
                    L.check(lib.kzv_stream_encode(self._h, chunk.data_ptr(), d, a, st), "stream_encode")
                    a += k
                L.check(lib.kzv_stream_start(self._h, st), "stream_start")
                bound = ST.step_bound(n, slots, Lh)
                fin, took, pads = C.c_int32(0), C.c_int32(0), C.c_int32(0)
                steps = 0
                while True:
                    L.check(lib.kzv_stream_step(self._h, 1 if graph else 0, st), "stream_step")
                    steps += 1
                    if steps % 8 == 0 or steps >= bound:          # the host only looks: selection and seating are the device's
                        if beams:
                            L.check(lib.kzv_stream_poll_beams(self._h, C.byref(fin), C.byref(took), C.byref(pads), st), "stream_poll_beams")
                        else:
                            L.check(lib.kzv_stream_poll(self._h, C.byref(fin), C.byref(took), st), "stream_poll")
                        if fin.value >= n:
                            break
                        if steps >= bound:
                            raise L.KzvError(f"generate_stream: {fin.value} of {n} lines ended after {steps} steps; {slots} slots bound them by {bound}")
                self.last_stream_steps += took.value
                keep += [ids] + [x for x in (lp, score, limd, alt_ids, alt_lp) if x is not None] + (nbo.tensors() if nbo is not None else [])
        finally:
            self.training = was
        if beams and pads.value:                                  # a running beam held padding: the slots' positions and key flags were wrong for it
            self.last_stream_pad_fallbacks += pads.value
            return static_beams(px, Lh, slots, lim, beams, ctl, lmr)
        if pfx is not None and pfx.forced_logprob is not None:
            self._wave_forced_lp = pfx.forced_logprob
        if nbo is not None:
            return nbo.result()
        if top_k:
            return ids, lp, (alt_ids, alt_lp)
        return ids, (score if beams else lp)

    def recognize_many(self, pixel_values, top_k: int = 0, n_best: int = 0, prefix_ids=None, prefix_texts=None, prefix_logprobs: bool = False,
                       **kw) -> list[dict]:
        """``generate_stream`` with its own log-probabilities: per image a dict of ``text``, ``tokens`` (ids without BOS / EOS / PAD),
        ``token_strings``, ``logprobs`` and ``confidence`` = exp(mean log-probability over the tokens, EOS included) -- ``recognize``'s
        definitions, for greedy decoding, with no teacher-forced second pass.  It returns NO centroids or peak patches: those come
        from the cross-attention maps of a teacher-forced pass, which ``recognize`` runs.  ``kw``: generate_stream's arguments; with
        ``top_k`` in 1..8 every record also holds ``alternatives`` and ``margins`` (build_records), taken from the stream's own steps.
        The generation controls (``no_repeat_ngram_size``, ``repetition_penalty``, ``min_length``, ``suppress_tokens``, ``allowed_tokens``)
        go through ``kw``; log-probabilities, confidence and alternatives are then those of the processed rows (generate_stream).
        So do ``lm`` / ``lm_weight`` (language-model fusion): the values are then those of the fused rows.
        ``num_beams`` > 1 (through ``kw``) with ``n_best`` n in 1..num_beams (default 1): the records of a beam search, from the winner's
        own search log-probabilities with no second pass, plus ``score`` (HF ``sequences_scores``) and ``hypotheses``: the n best
        readings of the line as such records, best first, the winner included as entry 0 (kzv/nbest.py).
        ``prefix_ids`` / ``prefix_texts`` (``recognize``'s; one entry per image of the whole call): forced prefixes.  The greedy records
        then hold ``forced``; their ``logprobs`` are exactly 0 at forced tokens (the forced row's), ``confidence`` is taken over the
        free tokens only and the ``alternatives`` of forced positions are empty; ``prefix_logprobs=True`` adds ``prefix_logprobs``, the
        model's own log-probability of every forced token (generate_stream(return_prefix_logprobs=True))."""
        import numpy as np
        from . import align as A
        from . import nbest as NB
        from . import prefix as PF
        c = self.cfg
        top_k = int(top_k)
        nb = int(kw.get("num_beams", 1))
        if prefix_texts is not None:
            if prefix_ids is not None:
                raise ValueError("recognize_many: prefix_ids or prefix_texts, not both")
            prefix_ids = PF.texts_to_ids(self.tokenizer, prefix_texts)
        forced = None
        if prefix_ids is not None:
            got = PF.normalise(prefix_ids, len(prefix_ids), vocab=c.vocab, pad_id=c.pad_id, bos_id=c.bos_id, eos_id=c.eos_id,
                               max_length=min(int(kw.get("max_length", 128)), c.max_pos - c.pad_id - 1), limits=kw.get("limits"))
            forced = [0] * len(prefix_ids) if got is None else got[1].tolist()
            kw = dict(kw, prefix_ids=prefix_ids)
        want_pl = bool(prefix_logprobs) and forced is not None and any(forced)
        if prefix_logprobs and (nb > 1 or n_best):
            raise ValueError("recognize_many: prefix_logprobs is served for greedy decoding")
        if nb > 1 or n_best:
            n = NB.check_request(nb, n_best or 1, True, "recognize_many")
            if nb == 1:
                raise ValueError("recognize_many: n_best needs a beam search (num_beams > 1)")
            gen, score, lp = self.generate_stream(pixel_values, return_logprobs=True, return_scores=True, top_k=top_k, num_return_sequences=n, **kw)
            recs = NB.records(self, gen, score, lp, n)
            if forced is not None:                # (a beam record's confidence still averages the forced tokens' exact zeros in)
                for r, f in zip(recs, forced):
                    r["forced"] = int(f)
            return recs
        alts = pl = None
        if top_k:
            gen, lp, a_ids, a_lp, *rest = self.generate_stream(pixel_values, return_logprobs=True, top_k=top_k, return_prefix_logprobs=want_pl, **kw)
            alts = (a_ids[:, 1:].cpu().numpy(), a_lp[:, 1:].cpu().numpy())
        else:
            gen, lp, *rest = self.generate_stream(pixel_values, return_logprobs=True, return_prefix_logprobs=want_pl, **kw)
        if want_pl:
            pl = rest[0].cpu().numpy()
        ids = gen.cpu().numpy()
        B, W = ids.shape
        tok = self.tokenizer
        recs = A.build_records(ids, lp[:, 1:].cpu().numpy(), np.zeros((B, W - 1, 2)), np.zeros((B, W - 1), dtype=np.int64),
                               pad_id=c.pad_id, bos_id=c.bos_id, eos_id=c.eos_id,
                               texts=None if tok is None else tok.batch_decode(gen, skip_special_tokens=True),
                               to_strings=None if tok is None else tok.convert_ids_to_tokens, alternatives=alts, forced=forced,
                               prefix_logprobs=pl)
        for r in recs:
            del r["centroids"], r["peak_patches"]
        return recs

    # ------------------------------------------------------------------ evaluation on the device (kzv/metrics.py)
    @property
    def one_char_tokenizer(self) -> bool:
        """Whether the tokenizer is one character per token (metrics.is_one_char_tokenizer), i.e. whether the id-level edit distance
        equals the reference's string-level one.  Checked once per model; False without a tokenizer."""
        if getattr(self, "_one_char", None) is None:
            from . import metrics as M
            self._one_char = self.tokenizer is not None and bool(M.is_one_char_tokenizer(self.tokenizer))
        return self._one_char

    def _edit_special_ids(self) -> list[int]:
        if self.tokenizer is None:             # no tokenizer to ask: the specials the geometry names
            return sorted({self.cfg.pad_id, self.cfg.bos_id, self.cfg.eos_id})
        if not self.one_char_tokenizer:
            raise ValueError("the device evaluation needs a tokenizer of one character per token with at most 8 specials; "
                             "score this model's lines with batch_decode + calculate_cer")
        return [int(i) for i in self.tokenizer.all_special_ids]

    def cer_of(self, generated_ids, labels) -> list[float]:
        """Per-line CER of ``generated_ids`` [N, <= 128] against ``labels`` [N, <= 128], computed from the ids on the device (one
        kzv_edit_distance, the distance-only kernel): the values ``calculate_cer`` returns for the two ``batch_decode``d strings, ==."""
        import torch
        from . import metrics as M
        gen = torch.as_tensor(generated_ids).to(self.device)
        st = M.edit_stats(gen, torch.as_tensor(labels).to(self.device), self._edit_special_ids(), self.cfg.vocab, ops=False)
        return M.cer_values(st["dist"], st["ref_len"], st["pred_len"])

    def evaluate_many(self, pixel_values, labels, num_beams: int = 1, top: int = 20, n_best: int = 0, **generate_stream_kw) -> dict:
        """``generate_stream`` over the images followed by ONE kzv_edit_distance against ``labels`` ([N, <= 128] ids, or an iterable of
        such batches in the images' order).  Returns ``cer`` (the mean of the per-line CER: the reference's test_cer), ``cer_corpus``
        (sum of distances / sum of label lengths), ``exact`` (share of lines with distance 0), ``substitutions`` / ``deletions`` /
        ``insertions`` / ``ref_chars`` (totals), ``per_line`` (numpy arrays ``cer``, ``dist``, ``ref_len``, ``pred_len``, ``ops``),
        ``characters`` (metrics.character_table: the ``top`` characters with the most errors) and ``ids`` (the generated rows).  The
        same call serves geometries where generate_stream runs ``generate``: it needs only the ids.  The generation controls of
        generate_stream (``no_repeat_ngram_size=3`` is what the stock TrOCR generation configs ship with) pass through its keywords, and
        so do ``lm`` / ``lm_weight`` (kzv.lm.sweep_weight picks the weight with this call) and ``prefix_ids`` (forced prefixes: with the
        first k label characters of every line forced, the CER of the rest separates early-error propagation from plain misreading;
        the forced characters are part of the scored rows).
        ``n_best`` n in 1..num_beams (beams only): the decode returns the n best readings of every line and ONE more kzv_edit_distance
        (distance only) scores them all; every key above stays the winner's, and the call adds ``cer_oracle`` (the mean over lines of the
        best reading's CER: what a rescoring of the candidates could reach at most), ``cer_oracle_corpus``, ``oracle_rank`` (how often
        rank r held the best reading, ties to the lower rank), ``per_line["dist_nbest"]`` [N, n] and ``per_line["cer_oracle"]`` [N] (kzv/nbest.py:
        oracle_stats)."""
        import numpy as np
        import torch
        from . import metrics as M
        from . import nbest as NB
        n_best = int(n_best)
        if n_best:
            NB.check_request(num_beams, n_best, False, "evaluate_many")
            if int(num_beams) == 1:
                raise ValueError("evaluate_many: n_best needs a beam search (num_beams > 1)")
        special = self._edit_special_ids()
        for k in ("return_logprobs", "return_scores", "top_k"):
            if generate_stream_kw.get(k):
                raise ValueError(f"evaluate_many scores the ids only: {k} is not served")
        gen_all = None
        if n_best:
            gen_all = self.generate_stream(pixel_values, num_beams=num_beams, num_return_sequences=n_best, **generate_stream_kw)
            gen = gen_all[0::n_best]
            gen = gen[:, :max(2, int((gen != self.cfg.pad_id).sum(dim=1).max()))]      # the winners at the width the call without n_best gives them
        else:
            gen = self.generate_stream(pixel_values, num_beams=num_beams, **generate_stream_kw)
        lab = labels if torch.is_tensor(labels) else torch.cat([torch.as_tensor(b) for b in labels])
        st = M.edit_stats(gen, lab.to(gen.device), special, self.cfg.vocab, char_stats=True)
        dist, ref_len, pred_len, ops = (st[k].cpu().numpy() for k in ("dist", "ref_len", "pred_len", "ops"))
        cers = M.cer_values(dist, ref_len, pred_len)
        tot = ops.astype(np.int64).sum(axis=0)
        chars = int(ref_len.astype(np.int64).sum())
        oracle, extra = {}, {}
        if gen_all is not None:
            oracle = NB.oracle_of_ids(self, gen_all, lab, n_best)
            extra = {"dist_nbest": oracle.pop("dist_nbest"), "cer_oracle": np.asarray(oracle.pop("cer_oracle_lines"), dtype=np.float64)}
        return {**oracle,
                "cer": sum(cers) / len(cers) if cers else 0.0,
                "cer_corpus": int(dist.astype(np.int64).sum()) / chars if chars else 0.0,
                "exact": float((dist == 0).mean()) if len(cers) else 0.0,
                "substitutions": int(tot[1]), "deletions": int(tot[2]), "insertions": int(tot[3]), "ref_chars": chars,
                "per_line": {"cer": np.asarray(cers, dtype=np.float64), "dist": dist, "ref_len": ref_len, "pred_len": pred_len, "ops": ops, **extra},
                "characters": M.character_table(st["char_stats"], self.tokenizer, top=top), "ids": gen}

    # ------------------------------------------------------------------ Lightning-shaped steps (:323-398)
    def training_step(self, batch, batch_idx):
        loss, _ = self.forward_loss(batch["pixel_values"], batch["labels"], want_logits=False)
        self.backward()
        self.last_loss = loss
        return loss

    def validation_step(self, batch, batch_idx):
        was = self.training
        self.training = False
        loss, _ = self.forward_loss(batch["pixel_values"], batch["labels"])
        val = float(loss.item())
        self.log("val_loss", val)
        if batch_idx < 5 and self.tokenizer is not None:
            # trocr_model.py:345-358: self(pixel_values) = beam-4 generation of the whole batch, CER of sample 0
            gen = self(batch["pixel_values"])["generated_ids"]
            pred = self.tokenizer.batch_decode(gen, skip_special_tokens=True)
            tgt = self.tokenizer.batch_decode(batch["labels"], skip_special_tokens=True)
            if len(pred) > 0 and len(tgt) > 0:
                self.log("val_cer", self.calculate_cer(pred[0], tgt[0]))
        self.training = was
        return val

    def test_step(self, batch, batch_idx):
        was = self.training
        self.training = False
        loss, _ = self.forward_loss(batch["pixel_values"], batch["labels"])
        val = float(loss.item())
        self.log("test_loss", val)
        if self.tokenizer is not None:
            gen = self(batch["pixel_values"])["generated_ids"]           # trocr_model.py:373: beam 4, max_length 128
            preds = self.tokenizer.batch_decode(gen, skip_special_tokens=True)
            tgts = self.tokenizer.batch_decode(batch["labels"], skip_special_tokens=True)
            cers = [self.calculate_cer(p, t) for p, t in zip(preds, tgts)]
            self.log("test_cer", sum(cers) / len(cers) if cers else 0.0)
        self.training = was
        return val

    def calculate_cer(self, pred_text: str, target_text: str) -> float:
        """Character Error Rate (trocr_model.py:400-410): Levenshtein / len(target)."""
        if len(target_text) == 0:
            return 1.0 if len(pred_text) > 0 else 0.0
        return _levenshtein(pred_text, target_text) / len(target_text)

    def configure_optimizers(self):
        from .optim import RAdamScheduleFree
        hp = self.hparams
        self._optimizer = RAdamScheduleFree(self, lr=hp.learning_rate, betas=(hp.beta1, hp.beta2), eps=hp.epsilon,
                                            weight_decay=hp.weight_decay)
        return self._optimizer

    # mode hooks (:423-451)
    def on_train_epoch_start(self):
        if self._optimizer is not None:
            self._optimizer.train()

    def on_validation_epoch_start(self):
        if self._optimizer is not None:
            self._optimizer.eval()

    def on_validation_epoch_end(self):
        if self._optimizer is not None:
            self._optimizer.train()

    def on_test_epoch_start(self):
        if self._optimizer is not None:
            self._optimizer.eval()

    def on_predict_epoch_start(self):
        if self._optimizer is not None:
            self._optimizer.eval()

    def decode_predictions(self, pixel_values) -> list[str]:
        self.eval()
        gen = self(pixel_values)["generated_ids"]                         # trocr_model.py:457
        return self.tokenizer.batch_decode(gen, skip_special_tokens=True)


def _levenshtein(a: str, b: str) -> int:
    if len(a) < len(b):
        a, b = b, a
    prev = list(range(len(b) + 1))
    for i, ca in enumerate(a, 1):
        cur = [i]
        for j, cb in enumerate(b, 1):
            cur.append(min(prev[j] + 1, cur[j - 1] + 1, prev[j - 1] + (ca != cb)))
        prev = cur
    return prev[-1]
