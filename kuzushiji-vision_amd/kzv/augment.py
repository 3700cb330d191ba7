"""Training-time augmentation of line crops, computed on the device (include/kzv.h, csrc/augment.hip).

The vocabulary is the reference workspace's own: `T.RandomAffine(degrees=7, translate=(0.07, 0.07), scale=(0.93, 1.07),
shear=(-5, 5, -5, 5))` (scripts/train_stackganv2_bcr_char.py:54); rotation, brightness / contrast, noise and blur with
p = 0.5 / 0.5 / 0.3 / 0.2 (src/utils/augmentation.py:35-98); the TrOCR recipe's stroke dilation and erosion.

The host draws one small parameter struct per crop (`sample_params`: numpy Philox, a pure function of seed, rank, epoch and step,
no GPU needed); `DeviceAugment` applies a batch of them in one launch of `kzv_augment_lines`; `AugmentLoader` wraps a training
loader.  Off unless asked for: `data.make_loader(..., augment=None)` builds no wrapper.
"""
from __future__ import annotations

import dataclasses
import math

import numpy as np

from . import _lib as L

# kzv_augment_params (72 bytes)
PARAMS_DTYPE = np.dtype([("m", "<f4", (6,)), ("blur", "<f4", (7,)), ("contrast", "<f4"), ("brightness", "<f4"),
                         ("noise_sigma", "<f4"), ("noise_key", "<u4"), ("morph", "<i4")])
assert PARAMS_DTYPE.itemsize == 72

IDENTITY_M = (1.0, 0.0, 0.0, 0.0, 1.0, 0.0)
IDENTITY_BLUR = (0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0)


@dataclasses.dataclass(frozen=True)
class AugmentConfig:
    """Ranges and probabilities.  Every operation tosses its own coin; one that loses gets exact identity parameters.

    degrees: rotation angle ~ U(-degrees, degrees).  translate = (a, b): shifts ~ U(-a*W, a*W), U(-b*H, b*H), rounded to whole
    pixels like torchvision's RandomAffine.  scale = (lo, hi).  shear = (x_lo, x_hi, y_lo, y_hi) in degrees.
    blur_sigma = (lo, hi) in pixels (7 taps).  brightness b, contrast c: Albumentations' RandomBrightnessContrast on [0, 1] pixels,
    p' = alpha*p + beta with alpha ~ 1 + U(-c, c), beta ~ U(-b, b); on the engine's [-1, 1] pixels that is
    v' = alpha*v + (alpha - 1 + 2*beta).  noise_sigma = (lo, hi) in [-1, 1] pixel units."""
    degrees: float = 0.0
    translate: tuple = (0.0, 0.0)
    scale: tuple = (1.0, 1.0)
    shear: tuple = (0.0, 0.0, 0.0, 0.0)
    p_affine: float = 0.0
    p_thin: float = 0.0
    p_thick: float = 0.0
    blur_sigma: tuple = (0.5, 1.5)
    p_blur: float = 0.0
    brightness: float = 0.0
    contrast: float = 0.0
    p_photometric: float = 0.0
    noise_sigma: tuple = (0.0, 0.0)
    p_noise: float = 0.0

    @property
    def enabled(self) -> bool:
        return any(p > 0 for p in (self.p_affine, self.p_thin, self.p_thick, self.p_blur, self.p_photometric, self.p_noise))


# GaussNoise's default var_limit (10, 50) on 0..255 pixels, as a standard deviation on [-1, 1] pixels
_NOISE = (2.0 * math.sqrt(10.0) / 255.0, 2.0 * math.sqrt(50.0) / 255.0)
PRESETS = {
    "off": AugmentConfig(),
    "reference": AugmentConfig(degrees=7.0, translate=(0.07, 0.07), scale=(0.93, 1.07), shear=(-5.0, 5.0, -5.0, 5.0), p_affine=0.5,
                               p_thin=0.1, p_thick=0.1, blur_sigma=(0.5, 1.5), p_blur=0.2, brightness=0.2, contrast=0.2,
                               p_photometric=0.5, noise_sigma=_NOISE, p_noise=0.3),
}


def preset(name: str) -> AugmentConfig:
    if name not in PRESETS:
        raise ValueError(f"unknown augmentation preset {name!r}: one of {sorted(PRESETS)}")
    return PRESETS[name]


def inverse_affine(angle, translate, scale, shear, H: int, W: int) -> np.ndarray:
    """float64 [..., 6]: output pixel -> source pixel in pixel-index units, for the forward transform torchvision's RandomAffine
    composes about the centre ((W-1)/2, (H-1)/2): translate, rotate, shear, scale (its _get_inverse_affine_matrix, restated).
    Scalars, or arrays of one shape for a batch."""
    rot, sx, sy = np.radians(np.asarray(angle, np.float64)), np.radians(np.asarray(shear[0], np.float64)), np.radians(np.asarray(shear[1], np.float64))
    scale = np.asarray(scale, np.float64)
    cx, cy = (W - 1) * 0.5, (H - 1) * 0.5
    tx, ty = np.asarray(translate[0], np.float64), np.asarray(translate[1], np.float64)
    a = np.cos(rot - sy) / np.cos(sy)
    b = -np.cos(rot - sy) * np.tan(sx) / np.cos(sy) - np.sin(rot)
    c = np.sin(rot - sy) / np.cos(sy)
    d = -np.sin(rot - sy) * np.tan(sx) / np.cos(sy) + np.cos(rot)
    m0, m1, m3, m4 = d / scale, -b / scale, -c / scale, a / scale
    m2 = m0 * (-cx - tx) + m1 * (-cy - ty) + cx
    m5 = m3 * (-cx - tx) + m4 * (-cy - ty) + cy
    return np.stack(np.broadcast_arrays(m0, m1, m2, m3, m4, m5), -1)


def blur_weights(sigma) -> np.ndarray:
    """float64 [..., 7]: Gaussian taps at -3 .. 3, normalised in double"""
    k = np.arange(-3, 4, dtype=np.float64)
    w = np.exp(-(k * k) / (2.0 * np.asarray(sigma, np.float64)[..., None] ** 2))
    return w / w.sum(-1, keepdims=True)


def identity_params(n: int) -> np.ndarray:
    p = np.zeros(n, PARAMS_DTYPE)
    p["m"], p["blur"], p["contrast"] = IDENTITY_M, IDENTITY_BLUR, 1.0
    return p


def draw_variates(n: int, seed: int, rank: int = 0, epoch: int = 0, step: int = 0):
    """(uniforms float64 [n, 16], noise keys uint64 [n]) of one batch.  Philox with key (seed, rank) and the 256-bit counter
    (0, 0, step, epoch), least significant word first: the generator advances the counter from its LOW word, one per block of four
    64-bit outputs, so `step` and `epoch` sit in the two HIGH words, which no draw of fewer than 2^128 blocks ever reaches.  Each
    (seed, rank, epoch, step) therefore owns a stream that no other one runs into.  (With `epoch` in the low word the stream of
    epoch e + 4 would be that of epoch e advanced by one crop.)"""
    mask = (1 << 64) - 1
    rng = np.random.Generator(np.random.Philox(key=[int(seed) & mask, int(rank) & mask], counter=[0, 0, int(step) & mask, int(epoch) & mask]))
    return rng.random((n, 16)), rng.integers(0, 1 << 32, size=n, dtype=np.uint64)


def sample_params(cfg: AugmentConfig, n: int, H: int, W: int, seed: int, rank: int = 0, epoch: int = 0, step: int = 0) -> np.ndarray:
    """n parameter structs for [n, 3, H, W] crops: deterministic in exactly (cfg, n, H, W, seed, rank, epoch, step), one disjoint
    Philox stream per (seed, rank, epoch, step) (`draw_variates`); every crop consumes the same number of variates whatever its
    coins say."""
    u, keys = draw_variates(n, seed, rank, epoch, step)
    out = identity_params(n)

    def span(lo, hi, x):
        return lo + (hi - lo) * x

    on = u[:, 0] < cfg.p_affine
    tx = np.round(span(-cfg.translate[0] * W, cfg.translate[0] * W, u[:, 2]))          # whole pixels, like torchvision
    ty = np.round(span(-cfg.translate[1] * H, cfg.translate[1] * H, u[:, 3]))
    m = inverse_affine(span(-cfg.degrees, cfg.degrees, u[:, 1]), (tx, ty), span(cfg.scale[0], cfg.scale[1], u[:, 4]),
                       (span(cfg.shear[0], cfg.shear[1], u[:, 5]), span(cfg.shear[2], cfg.shear[3], u[:, 6])), H, W)
    out["m"][on] = m[on]                                                               # rounded once, here, to fp32
    out["morph"] = np.where(u[:, 7] < cfg.p_thin, 1, np.where(u[:, 7] < cfg.p_thin + cfg.p_thick, 2, 0))
    on = u[:, 8] < cfg.p_blur
    out["blur"][on] = blur_weights(span(cfg.blur_sigma[0], cfg.blur_sigma[1], u[:, 9]))[on]
    on = u[:, 10] < cfg.p_photometric
    alpha = 1.0 + span(-cfg.contrast, cfg.contrast, u[:, 11])
    beta = span(-cfg.brightness, cfg.brightness, u[:, 12])
    out["contrast"][on], out["brightness"][on] = alpha[on], (alpha - 1.0 + 2.0 * beta)[on]
    on = u[:, 13] < cfg.p_noise
    out["noise_sigma"][on] = span(cfg.noise_sigma[0], cfg.noise_sigma[1], u[:, 14])[on]
    out["noise_key"][on] = keys[on]
    return out


class DeviceAugment:
    """pixel_values [n, 3, H, W] fp32 on the GPU + n parameter structs -> the augmented batch (a new tensor, or `out`)."""

    def __init__(self, device="cuda"):
        import torch
        d = torch.device(device)
        if d.type == "cuda" and d.index is None:    # "cuda" and "cuda:0" compare unequal: name the card once
            d = torch.device("cuda", torch.cuda.current_device())
        self.device = d
        self._keep = None

    def __call__(self, pixel_values, params, out=None):
        import torch
        px = pixel_values
        if not torch.is_tensor(px) or px.dim() != 4 or px.shape[1] != 3 or px.dtype != torch.float32 or not px.is_cuda:
            raise ValueError("pixel_values must be a [n, 3, H, W] float32 tensor on the GPU")
        px = px.contiguous()
        n, _, H, W = px.shape
        params = np.ascontiguousarray(params, PARAMS_DTYPE)
        if params.shape != (n,):
            raise ValueError(f"{params.shape} parameter structs for a batch of {n}")
        if out is None:
            out = torch.empty_like(px)
        elif out.shape != px.shape or out.dtype != torch.float32 or out.device != px.device or not out.is_contiguous():
            raise ValueError("out must be a contiguous float32 tensor of pixel_values' shape on its device")
        d_params = torch.from_numpy(params.view(np.uint8).reshape(-1).copy()).to(px.device, non_blocking=True)
        L.check(L.load().kzv_augment_lines(px.data_ptr(), d_params.data_ptr(), n, H, W, out.data_ptr(), L.stream_handle()), "augment_lines")
        self._keep = (px, d_params)                # the staging tensors must outlive the asynchronous kernel
        return out


class AugmentLoader:
    """Wraps a training loader: every batch leaves with `pixel_values` on the device and augmented; labels and every other key pass
    through.  `step` is the batch's index within the current pass (it restarts at 0 in every `__iter__`), `epoch` is what `set_epoch`
    last said and nothing else moves it: together with seed and rank they key the parameters, so a run repeats exactly and no two
    ranks, epochs or steps share a draw.  The other side of that: a second pass WITHOUT a `set_epoch` in between repeats the first
    pass's draws on purpose (it is not a fresh draw per pass), and a pass that resumes in the middle of an epoch counts its steps
    from 0 again.  `kzv.trainer.fit` calls `set_epoch` before every epoch; a caller with a loop of their own must do the same."""

    def __init__(self, loader, augment: DeviceAugment, cfg: AugmentConfig, seed: int = 42, rank: int = 0):
        self.loader, self.augment, self.cfg, self.seed, self.rank = loader, augment, cfg, int(seed), int(rank)
        self.epoch, self.step = 0, 0

    def __len__(self):
        return len(self.loader)

    def set_epoch(self, epoch):
        self.epoch = int(epoch)
        if hasattr(self.loader, "set_epoch"):
            self.loader.set_epoch(epoch)

    def __iter__(self):
        import torch
        self.step = 0
        for batch in self.loader:
            px = batch["pixel_values"]
            if px.device != self.augment.device or px.dtype != torch.float32:
                px = px.to(self.augment.device, dtype=torch.float32, non_blocking=True)
            n, _, H, W = px.shape
            params = sample_params(self.cfg, n, H, W, self.seed, self.rank, self.epoch, self.step)
            out = dict(batch)
            out["pixel_values"] = self.augment(px, params)
            self.step += 1
            yield out
