// Training-time augmentation of line crops on the device (include/kzv.h, "training-time augmentation of line crops").
//
// One launch over a batch [n, 3, H, W]: affine warp (bilinear, +1 fill) -> 3x3 stroke morphology -> separable 7-tap blur ->
// contrast / brightness / hashed noise -> clamp.  A 256-thread workgroup owns one TH x TW output tile of one channel of one image.
//
// A crop that drew neither blur nor morphology (two in three under the reference preset) needs no neighbourhood: each thread warps
// its own pixels and stores them, no LDS, no barrier.  The others walk the stages through two LDS images of the tile plus a halo
// of up to 4 (1 for the morphology, 3 for the blur):
//
//   A  = warp at every position of tile + halo, taken at coordinates CLAMPED to the canvas, so the image is the warped canvas
//        extended by replication.  For a 3x3 max / min around an in-canvas centre, replication equals "skip the neighbours
//        outside"; for the blur it is the replicate rule itself.
//   B  = morphology of A at tile + blur halo, around the CLAMPED centre (so B is replicate-extended too)
//   Hb = horizontal blur of B at the tile's columns and tile + blur halo rows
//   out = vertical blur of Hb from a register column, photometric, noise, one coalesced store per row
//
// Which stages run is block-uniform (the parameters are per image) and exact: the identity blur {0,0,0,1,0,0,0} and
// noise_sigma = 0 add zeros, and a map that is a whole-pixel shift (the identity included) has fx = fy = 0, so its one tap IS the
// bilinear result.  The source is read about once (neighbouring taps and tiles meet in L1 / L2), the output written once:
// 2 * n*3*H*W*4 bytes.  Offsets inside a plane fit 32 bits (3*H*W < 2^32): uniform base + 32-bit lane offset addressing.
#include "kzv_common.h"
#include "../../include/kzv.h"
#include "kzv_host.h"

namespace {

constexpr int TH = 32, TW = 64;                 // output tile: one wave per row of TW, 4 waves
constexpr int HALO = 4;
constexpr int SA = TW + 2 * HALO;               // row stride of an LDS image (72 floats: consecutive lanes, consecutive banks)
constexpr int IMG = (TH + 2 * HALO) * SA;       // floats per LDS image
constexpr int ROWS_PER_WAVE = TH / 4;

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return min(max(v, lo), hi); }

// the warped canvas at output pixel (gx, gy), both inside the canvas
template <bool SHIFT>
__device__ __forceinline__ float warp_at(const float* __restrict__ src, const kzv_augment_params& p, int gx, int gy, int H, int W) {
    const float xf = (float)gx, yf = (float)gy;
    float sx = fmaf(p.m[0], xf, fmaf(p.m[1], yf, p.m[2]));
    float sy = fmaf(p.m[3], xf, fmaf(p.m[4], yf, p.m[5]));
    sx = fminf(fmaxf(sx, -1.f), (float)W);          // beyond these every tap is fill; nothing huge becomes an integer
    sy = fminf(fmaxf(sy, -1.f), (float)H);
    if (SHIFT) {                                    // whole-pixel shift: sx, sy are integers, the first tap is the result
        const int ix = (int)sx, iy = (int)sy;
        const float l = src[(unsigned)clampi(iy, 0, H - 1) * (unsigned)W + (unsigned)clampi(ix, 0, W - 1)];
        return ((unsigned)ix < (unsigned)W && (unsigned)iy < (unsigned)H) ? l : 1.f;
    }
    const float flx = floorf(sx), fly = floorf(sy);
    const float fx = sx - flx, fy = sy - fly;
    const int ix = (int)flx, iy = (int)fly;         // -1 .. W, -1 .. H
    const bool vx0 = (unsigned)ix < (unsigned)W, vx1 = (unsigned)(ix + 1) < (unsigned)W;
    const bool vy0 = (unsigned)iy < (unsigned)H, vy1 = (unsigned)(iy + 1) < (unsigned)H;
    const unsigned cx0 = (unsigned)clampi(ix, 0, W - 1), cx1 = (unsigned)clampi(ix + 1, 0, W - 1);
    const unsigned ro0 = (unsigned)clampi(iy, 0, H - 1) * (unsigned)W, ro1 = (unsigned)clampi(iy + 1, 0, H - 1) * (unsigned)W;
    // clamped addresses, then select the fill: no branch around a load
    const float l00 = src[ro0 + cx0], l01 = src[ro0 + cx1], l10 = src[ro1 + cx0], l11 = src[ro1 + cx1];
    const float a = (vy0 && vx0) ? l00 : 1.f, b = (vy0 && vx1) ? l01 : 1.f;
    const float c = (vy1 && vx0) ? l10 : 1.f, d = (vy1 && vx1) ? l11 : 1.f;
    const float top = a + fx * (b - a), bot = c + fx * (d - c);
    return top + fy * (bot - top);
}

// contrast / brightness / noise / clamp of the value at (gx, gy) of channel c
template <bool NOISE>
__device__ __forceinline__ float finish(float v, const kzv_augment_params& p, int c, int gx, int gy, int H, int W) {
    float o = fmaf(p.contrast, v, p.brightness);
    if (NOISE) {
        const unsigned e = ((unsigned)c * (unsigned)H + (unsigned)gy) * (unsigned)W + (unsigned)gx;
        const unsigned h = kzv_hash32(e * 0x9E3779B9U + p.noise_key);
        const int sum = (int)((h & 0xffu) + ((h >> 8) & 0xffu) + ((h >> 16) & 0xffu) + (h >> 24)) - 510;
        o = fmaf(p.noise_sigma, (float)sum * (1.f / 147.80f), o);
    }
    return fminf(fmaxf(o, -1.f), 1.f);
}

// no blur, no morphology: thread (col, wave) owns rows wave, wave + 4, ... of its column; nothing is shared
template <bool SHIFT, bool NOISE>
__device__ __forceinline__ void pointwise_tile(const float* __restrict__ src, float* __restrict__ dst, const kzv_augment_params& p, int c,
                                               int x0, int y0, int H, int W) {
    const int gx = x0 + (threadIdx.x & 63);
    if (gx >= W) return;
#pragma unroll
    for (int j = 0; j < ROWS_PER_WAVE; ++j) {
        const int gy = y0 + (threadIdx.x >> 6) + 4 * j;
        if (gy < H) dst[(unsigned)gy * (unsigned)W + (unsigned)gx] = finish<NOISE>(warp_at<SHIFT>(src, p, gx, gy, H, W), p, c, gx, gy, H, W);
    }
}

// stage 1 of the LDS path: (TH + 2 ha) x (TW + 2 ha) positions into image A at (row + HALO, col + HALO)
template <bool SHIFT>
__device__ __forceinline__ void fill_warped(float* lds, const float* __restrict__ src, const kzv_augment_params& p, int ha, int x0, int y0,
                                            int H, int W) {
    const int wr = TW + 2 * ha, cnt = (TH + 2 * ha) * wr;
    const unsigned rcp = ((1u << 20) + wr - 1) / wr;           // idx / wr = (idx * rcp) >> 20, exact while idx * wr < 2^20
    for (int idx = threadIdx.x; idx < cnt; idx += 256) {
        const int r = (int)(((unsigned)idx * rcp) >> 20), cc = idx - r * wr;
        const int gy = clampi(y0 + r - ha, 0, H - 1), gx = clampi(x0 + cc - ha, 0, W - 1);
        lds[(r + HALO - ha) * SA + cc + HALO - ha] = warp_at<SHIFT>(src, p, gx, gy, H, W);
    }
}

// stage 2 of the LDS path: 3x3 maximum / minimum of image A into image B at tile + hb, around the CLAMPED centre: the canvas position
// clamp(y0 + r - hb) sits at image row clamp(...) - y0 + HALO
template <bool IS_MAX>
__device__ __forceinline__ void morph_stage(float* lds, int hb, int x0, int y0, int H, int W) {
    const int wr = TW + 2 * hb, cnt = (TH + 2 * hb) * wr;
    const unsigned rcp = ((1u << 20) + wr - 1) / wr;
    for (int idx = threadIdx.x; idx < cnt; idx += 256) {
        const int r = (int)(((unsigned)idx * rcp) >> 20), cc = idx - r * wr;
        const int ry = clampi(y0 + r - hb, 0, H - 1) - y0 + HALO, rx = clampi(x0 + cc - hb, 0, W - 1) - x0 + HALO;
        const float* q = lds + ry * SA + rx;
        float m[3];
#pragma unroll
        for (int dy = -1; dy <= 1; ++dy) {
            const float a = q[dy * SA - 1], b = q[dy * SA], c = q[dy * SA + 1];
            m[dy + 1] = IS_MAX ? fmaxf(fmaxf(a, b), c) : fminf(fminf(a, b), c);
        }
        lds[IMG + (r + HALO - hb) * SA + cc + HALO - hb] = IS_MAX ? fmaxf(fmaxf(m[0], m[1]), m[2]) : fminf(fminf(m[0], m[1]), m[2]);
    }
}

__global__ __launch_bounds__(256) void augment_kernel(const float* __restrict__ in, const kzv_augment_params* __restrict__ params,
                                                      float* __restrict__ out, int H, int W, int tiles_x, int tiles_y) {
    __shared__ float lds[2 * IMG];
    // block -> (image, channel, tile): all wave-uniform
    unsigned b = blockIdx.x;
    const int tx = (int)(b % (unsigned)tiles_x); b /= (unsigned)tiles_x;
    const int ty = (int)(b % (unsigned)tiles_y); b /= (unsigned)tiles_y;
    const int c = (int)(b % 3u);
    const int n = (int)(b / 3u);
    const kzv_augment_params p = params[n];     // block-uniform address: uniform loads
    const int x0 = tx * TW, y0 = ty * TH;
    const int64_t plane = (int64_t)H * W;
    const float* __restrict__ src = in + ((int64_t)n * 3 + c) * plane;
    float* __restrict__ dst = out + ((int64_t)n * 3 + c) * plane;
    const int tid = threadIdx.x;

    const bool do_blur = !(p.blur[0] == 0.f && p.blur[1] == 0.f && p.blur[2] == 0.f && p.blur[3] == 1.f && p.blur[4] == 0.f &&
                           p.blur[5] == 0.f && p.blur[6] == 0.f);
    const bool do_morph = p.morph == 1 || p.morph == 2;
    const bool do_noise = p.noise_sigma != 0.f;
    const bool shift = p.m[0] == 1.f && p.m[1] == 0.f && p.m[3] == 0.f && p.m[4] == 1.f && p.m[2] == floorf(p.m[2]) && p.m[5] == floorf(p.m[5]);

    if (!do_blur && !do_morph) {
        if (shift) {
            if (do_noise) pointwise_tile<true, true>(src, dst, p, c, x0, y0, H, W);
            else pointwise_tile<true, false>(src, dst, p, c, x0, y0, H, W);
        } else {
            if (do_noise) pointwise_tile<false, true>(src, dst, p, c, x0, y0, H, W);
            else pointwise_tile<false, false>(src, dst, p, c, x0, y0, H, W);
        }
        return;
    }

    const int hb = do_blur ? 3 : 0;             // halo the blur needs
    const int ha = hb + (do_morph ? 1 : 0);     // halo the warp fills
    int cur = 0;                                // float offset of the image the next stage reads

    // ---- 1. warp into A ----
    if (shift) fill_warped<true>(lds, src, p, ha, x0, y0, H, W);
    else fill_warped<false>(lds, src, p, ha, x0, y0, H, W);
    __syncthreads();

    // ---- 2. morphology into B at tile + hb ----
    if (do_morph) {
        if (p.morph == 1) morph_stage<true>(lds, hb, x0, y0, H, W);
        else morph_stage<false>(lds, hb, x0, y0, H, W);
        cur = IMG;
        __syncthreads();
    }

    // ---- 3a. horizontal blur into the other image: rows tile + 3, the tile's columns (lane = column) ----
    if (do_blur) {
        const int other = IMG - cur;
        for (int idx = tid; idx < (TH + 6) * TW; idx += 256) {
            const int r = idx >> 6, cc = idx & 63;
            const float* q = lds + cur + (r + HALO - 3) * SA + cc + HALO;
            float s = p.blur[0] * q[-3];
#pragma unroll
            for (int k = 1; k < 7; ++k) s = fmaf(p.blur[k], q[k - 3], s);
            lds[other + (r + HALO - 3) * SA + cc + HALO] = s;
        }
        cur = other;
        __syncthreads();
    }

    // ---- 3b + 4. vertical blur from a register column, photometric, noise, store: wave w owns rows w*8 .. w*8+7 ----
    const int col = tid & 63, row0 = (tid >> 6) * ROWS_PER_WAVE;
    const int gx = x0 + col;
    float v[ROWS_PER_WAVE];
    if (do_blur) {
        float h[ROWS_PER_WAVE + 6];
#pragma unroll
        for (int j = 0; j < ROWS_PER_WAVE + 6; ++j) h[j] = lds[cur + (row0 + j + HALO - 3) * SA + col + HALO];
#pragma unroll
        for (int j = 0; j < ROWS_PER_WAVE; ++j) {
            float s = p.blur[0] * h[j];
#pragma unroll
            for (int k = 1; k < 7; ++k) s = fmaf(p.blur[k], h[j + k], s);
            v[j] = s;
        }
    } else {
#pragma unroll
        for (int j = 0; j < ROWS_PER_WAVE; ++j) v[j] = lds[cur + (row0 + j + HALO) * SA + col + HALO];
    }
#pragma unroll
    for (int j = 0; j < ROWS_PER_WAVE; ++j) {
        const int gy = y0 + row0 + j;
        const float o = do_noise ? finish<true>(v[j], p, c, gx, gy, H, W) : finish<false>(v[j], p, c, gx, gy, H, W);
        if (gx < W && gy < H) dst[(unsigned)gy * (unsigned)W + (unsigned)gx] = o;
    }
}

}  // namespace

extern "C" int kzv_augment_lines(const float* in, const kzv_augment_params* params, int n, int H, int W, float* out, void* stream) {
    if (!in || !params || !out) return kzv_fail(KZV_E_ARG, "augment_lines: null operand");
    if (n < 1 || H < 1 || W < 1) return kzv_fail(KZV_E_ARG, "augment_lines: n, H and W must be positive (got %d, %d, %d)", n, H, W);
    if (3ll * H * W >= (1ll << 32)) return kzv_fail(KZV_E_ARG, "augment_lines: 3*H*W = %lld must stay below 2^32", 3ll * H * W);
    const int64_t tiles_x = (W + TW - 1) / TW, tiles_y = (H + TH - 1) / TH;
    const int64_t blocks = tiles_x * tiles_y * 3 * n;
    // a launch carries fewer than 2^32 threads: 256 per tile, so fewer than 2^24 tiles (32x64 pixels of one channel each)
    if (blocks * 256 >= (1ll << 32))
        return kzv_fail(KZV_E_ARG, "augment_lines: %lld tiles of 32x64 in one launch (tiles * 256 threads must stay below 2^32)", (long long)blocks);
    const int64_t bytes = (int64_t)n * 3 * H * W * (int64_t)sizeof(float);
    const uintptr_t a = (uintptr_t)in, o = (uintptr_t)out;
    if (a < o + (uintptr_t)bytes && o < a + (uintptr_t)bytes)
        return kzv_fail(KZV_E_ARG, "augment_lines: out overlaps in (the warp gathers; it cannot run in place)");
    hipLaunchKernelGGL(augment_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, in, params, out, H, W, (int)tiles_x,
                       (int)tiles_y);
    return kzv_check_launch("augment_lines");
}
