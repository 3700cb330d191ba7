"""fp64 CPU restatement of kzv_augment_lines (include/kzv.h): explicit numpy, stage by stage, in the contract's order.
tests/test_augment_cpu.py pins each stage to its torch statement; tests/test_augment_gpu.py holds the kernel to this file."""
import numpy as np

GOLD = np.uint32(0x9E3779B9)


def hash32(x):
    """kzv_hash32 (csrc/kzv_common.h) on a uint32 array"""
    x = np.asarray(x, np.uint32).copy()
    x ^= x >> np.uint32(16); x *= np.uint32(0x7feb352d)
    x ^= x >> np.uint32(15); x *= np.uint32(0x846ca68b)
    x ^= x >> np.uint32(16)
    return x


def noise_sums(key, H, W):
    """int64 [3, H, W]: b0 + b1 + b2 + b3 of hash32(e * GOLD + key), e = (c*H + y)*W + x"""
    e = np.arange(3 * H * W, dtype=np.uint32)
    h = hash32(e * GOLD + np.uint32(key))
    s = (h & np.uint32(0xff)).astype(np.int64) + ((h >> np.uint32(8)) & np.uint32(0xff)) + ((h >> np.uint32(16)) & np.uint32(0xff)) + (h >> np.uint32(24))
    return s.reshape(3, H, W)


def noise_g(key, H, W):
    return (noise_sums(key, H, W) - 510).astype(np.float64) * (1.0 / 147.80)


def source_coords(m, H, W):
    m = [float(v) for v in m]
    ys, xs = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    return m[0] * xs + m[1] * ys + m[2], m[3] * xs + m[4] * ys + m[5]


def warp(x, m):
    """x [3, H, W] float64; four bilinear taps, +1 outside the canvas"""
    _, H, W = x.shape
    sx, sy = source_coords(m, H, W)
    sx, sy = np.clip(sx, -1.0, W), np.clip(sy, -1.0, H)
    x0, y0 = np.floor(sx), np.floor(sy)
    fx, fy = sx - x0, sy - y0
    x0, y0 = x0.astype(np.int64), y0.astype(np.int64)

    def tap(iy, ix):
        ok = (ix >= 0) & (ix < W) & (iy >= 0) & (iy < H)
        return np.where(ok[None], x[:, np.clip(iy, 0, H - 1), np.clip(ix, 0, W - 1)], 1.0)

    a, b, c, d = tap(y0, x0), tap(y0, x0 + 1), tap(y0 + 1, x0), tap(y0 + 1, x0 + 1)
    top, bot = a + fx * (b - a), c + fx * (d - c)
    return top + fy * (bot - top)


def morph(x, mode):
    """3x3 maximum (1) / minimum (2) over the neighbours inside the canvas"""
    if mode == 0:
        return x
    _, H, W = x.shape
    pad = -np.inf if mode == 1 else np.inf
    xp = np.pad(x, ((0, 0), (1, 1), (1, 1)), constant_values=pad)
    views = [xp[:, dy:dy + H, dx:dx + W] for dy in range(3) for dx in range(3)]
    return np.maximum.reduce(views) if mode == 1 else np.minimum.reduce(views)


def blur(x, w):
    """7 taps along x, then along y, replicate at the canvas edge"""
    w = [float(v) for v in w]
    _, H, W = x.shape
    xp = np.pad(x, ((0, 0), (0, 0), (3, 3)), mode="edge")
    h = sum(w[k] * xp[:, :, k:k + W] for k in range(7))
    hp = np.pad(h, ((0, 0), (3, 3), (0, 0)), mode="edge")
    return sum(w[k] * hp[:, k:k + H, :] for k in range(7))


def augment_one(x, p):
    """x [3, H, W] (any float) + one kzv_augment_params record -> float64 [3, H, W]"""
    x = np.asarray(x, np.float64)
    _, H, W = x.shape
    v = blur(morph(warp(x, p["m"]), int(p["morph"])), p["blur"])
    o = float(p["contrast"]) * v + float(p["brightness"])
    if float(p["noise_sigma"]) != 0.0:
        o = o + float(p["noise_sigma"]) * noise_g(int(p["noise_key"]), H, W)
    return np.clip(o, -1.0, 1.0)


def augment(x, params):
    return np.stack([augment_one(x[i], params[i]) for i in range(len(params))])
