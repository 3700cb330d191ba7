"""TEST INFRASTRUCTURE (oracle side; never imported by the product path).

numpy statement of the hidden-state dropout generator of the HIP kernels (kuzushiji-vision_amd/csrc/kzv_common.h, "counter-based
dropout bits": drop_bits / drop_keep; threshold and multiplier from kzv_drop_params, csrc/host.cpp), the counterpart of
oracle/attn_dropout.py for every site that is not an attention-probability site: the GEMM residual epilogues, LayerNorm forward /
backward, the embedding assembly, the cast + column-sum kernel.  kzv_debug_dropout_mask, which the mask-replay tests trust, is
checked bit for bit against this file in tests/test_glue_ops_gpu.py.

One 32-bit hash per PAIR of consecutive elements, 16 bits per element (all arithmetic mod 2^32):
    e = row * ld_index + col,   x = mix(((e >> 1) * 0x9E3779B9) + key)          mix = kzv_hash32
    bits = high 16 bits of x if e is odd, else the low 16
    kept  iff  bits >= thr16,   thr16 = round(p * 65536) clamped to 1 .. 65535  (so P(drop) = thr16 / 65536; p <= 0: nothing drops)
    multiplier = 65536 / (65536 - thr16) in fp32 where kept, 0 where dropped
"""
import numpy as np

from oracle.attn_dropout import thr16_of


def hash32(x: np.ndarray) -> np.ndarray:
    """kzv_hash32 on a uint32 array."""
    u32 = np.uint32
    with np.errstate(over="ignore"):
        x = x ^ (x >> u32(16))
        x = x * u32(0x7feb352d)
        x = x ^ (x >> u32(15))
        x = x * u32(0x846ca68b)
        x = x ^ (x >> u32(16))
    return x


def bits16(key: int, rows: int, cols: int, ld_index: int) -> np.ndarray:
    """The 16-bit value of every element: uint32 array [rows, cols] holding values < 65536."""
    u32 = np.uint32
    r = (np.arange(rows, dtype=np.uint64) & 0xFFFFFFFF).astype(np.uint32)[:, None]
    c = (np.arange(cols, dtype=np.uint64) & 0xFFFFFFFF).astype(np.uint32)[None, :]
    with np.errstate(over="ignore"):
        e = r * u32(ld_index & 0xFFFFFFFF) + c
        x = hash32((e >> u32(1)) * u32(0x9E3779B9) + u32(key & 0xFFFFFFFF))
    return np.where((e & u32(1)) == 1, x >> u32(16), x & u32(0xffff))


def keep_mask(key: int, p: float, rows: int, cols: int, ld_index: int) -> np.ndarray:
    """bool [rows, cols]: True where the element is kept."""
    t = thr16_of(p)
    if t == 0:
        return np.ones((rows, cols), dtype=bool)
    return bits16(key, rows, cols, ld_index) >= t


def multiplier(key: int, p: float, rows: int, cols: int, ld_index: int) -> np.ndarray:
    """What kzv_debug_dropout_mask writes: 0 or 1 / P(keep) of the threshold actually used, fp32 [rows, cols]."""
    t = thr16_of(p)
    inv = np.float32(65536.0) / np.float32(65536 - t) if t else np.float32(1.0)
    return keep_mask(key, p, rows, cols, ld_index).astype(np.float32) * inv
