// Gradient clipping + RAdamScheduleFree step, fused over the flat fp32 buffers (HBM-bound:
// reads p, z, v, g and writes p, z, v once = 28 B / parameter).
// Replaces clip_grad_norm_(1.0) (scripts/train_trocr.py:175) and schedulefree.RAdamScheduleFree.step
// (src/models/trocr_model.py:412-421).  The per-step scalars (lr_t, c_{k+1}, bias correction) are
// computed on the host (kzv/optim.py) exactly as oracle/trocr_oracle.py::RAdamScheduleFreeState does.
#include "kzv_common.h"
#include "../../include/kzv.h"
#include "kzv_host.h"
#include "kzv_kernels.h"

namespace {

constexpr int NORM_BLOCKS = 1024;

__global__ __launch_bounds__(256) void sqnorm_partial_kernel(const float* __restrict__ g, int64_t n4, float* __restrict__ partial) {
    __shared__ float red[4];
    float s = 0.f;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (int64_t)gridDim.x * 256) {
        const float4 v = ((const float4*)g)[i];
        s += v.x * v.x + v.y * v.y + v.z * v.z + v.w * v.w;
    }
    s = wave_sum(s);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) partial[blockIdx.x] = red[0] + red[1] + red[2] + red[3];
}

__global__ __launch_bounds__(256) void sqnorm_final_kernel(const float* __restrict__ partial, int n, float* out) {
    __shared__ float red[4];
    float s = 0.f;
    for (int i = threadIdx.x; i < n; i += 256) s += partial[i];
    s = wave_sum(s);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) *out = red[0] + red[1] + red[2] + red[3];
}

// EMA: optional shadow parameters (src/callbacks/ema.py:51-58: shadow = decay * shadow + (1 - decay) * param after every
// batch) updated from the new parameters while they are still in registers -- one more 8-B/parameter stream instead of a
// separate 12-B/parameter pass over 98 M parameters.
template <bool EMA>
__global__ __launch_bounds__(256) void clip_step_kernel(float* __restrict__ p, float* __restrict__ z, float* __restrict__ v,
                                                        const float* __restrict__ g, int64_t n4,
                                                        const float* __restrict__ sqnorm, const kzv_opt_step s,
                                                        float* __restrict__ ema, const float ema_w) {
    // total norm of the SCALED grads; torch: coef = clamp(max_norm / (norm + 1e-6), max=1)
    float gs = s.grad_scale;
    if (s.max_grad_norm > 0.f) {
        const float norm = sqrtf(*sqnorm) * fabsf(s.grad_scale);
        gs *= fminf(1.f, s.max_grad_norm / (norm + 1e-6f));
    }
    const float ylr = s.lr_t * (s.beta1 * (1.f - s.ckp1) - 1.f);
    const float inv_bc2 = 1.f / s.bias_correction2;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (int64_t)gridDim.x * 256) {
        // z, v and the gradient are touched once per step: streaming loads / stores (the parameters stay plain: the weight casts read them next);
        // step 30.26 -> 30.20 ms over four same-box alternations
        auto ntl = [](const float* q, int64_t i) { const f32x4 t = __builtin_nontemporal_load((const f32x4*)q + i); return make_float4(t[0], t[1], t[2], t[3]); };
        float4 P = ((float4*)p)[i], Z = ntl(z, i), V = ntl(v, i);
        const float4 G4 = ntl(g, i);
        float* pp = (float*)&P; float* zz = (float*)&Z; float* vv = (float*)&V; const float* gg = (const float*)&G4;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const float gr = gg[r] * gs;
            vv[r] = vv[r] * s.beta2 + s.one_minus_beta2 * gr * gr;
            float gn = s.adaptive ? gr / (sqrtf(vv[r] * inv_bc2) + s.eps) : gr;
            gn += s.weight_decay * pp[r];
            float y = pp[r] + s.ckp1 * (zz[r] - pp[r]);
            y += ylr * gn;
            pp[r] = y;
            zz[r] -= s.lr_t * gn;
        }
        ((float4*)p)[i] = P;
        __builtin_nontemporal_store((f32x4){Z.x, Z.y, Z.z, Z.w}, (f32x4*)z + i); __builtin_nontemporal_store((f32x4){V.x, V.y, V.z, V.w}, (f32x4*)v + i);
        if (EMA) {
            float4 E = ((float4*)ema)[i];
            E.x += ema_w * (P.x - E.x); E.y += ema_w * (P.y - E.y); E.z += ema_w * (P.z - E.z); E.w += ema_w * (P.w - E.w);
            ((float4*)ema)[i] = E;
        }
    }
}

// ---- parameter groups (fine-tuning: layer-wise learning-rate decay, frozen ranges, weight-decay exemptions) ----------------------
// The table is sorted, contiguous and covers [0, n); every boundary is a multiple of 64 floats, so a float4 never straddles two groups.
// Both grouped kernels walk the buffer in the plain kernels' grid-stride order (the same addresses per workgroup and pass, hence the same
// HBM traffic pattern and, for the norm, the same sum order).  A lane's float index only grows, so it keeps the group it is in (its `hi`
// and the two scales, three registers) and looks the table up again only when it has left that group: a binary search over the groups
// behind the current one, 12 dependent loads at most from a table of <= 96 KiB that stays in the caches.  A table that does not cover
// [0, n) gives wrong scales for the uncovered tail but no access outside the table: the search is clamped to its last entry, and the
// accesses to p, z, v, g and the shadow are indexed by i < n4 alone.
struct GroupCursor {
    int gi = -1;
    int64_t hi = 0;            // floats; the cursor is valid for float indices < hi
    float lr_scale = 0.f, wd_scale = 0.f;
    __device__ __forceinline__ void seek(const kzv_opt_group* __restrict__ groups, const int n_groups, const int64_t f) {
        if (f < hi) return;
        int a = min(gi + 1, n_groups - 1), b = n_groups - 1;     // the first group whose hi is beyond f
        while (a < b) {
            const int mid = (a + b) >> 1;
            if (groups[mid].hi > f) b = mid; else a = mid + 1;
        }
        gi = a; hi = groups[a].hi; lr_scale = groups[a].lr_scale; wd_scale = groups[a].wd_scale;
    }
};

// sqnorm_partial_kernel over the trainable groups: a frozen group (lr_scale == 0) has no gradient as far as clip_grad_norm_ is concerned,
// its floats are not read.  The same blocks, the same order of additions per thread, the same folds: with one trainable group the bits of
// kzv_grad_sqnorm, and the same bits from run to run for any table.
__global__ __launch_bounds__(256) void sqnorm_groups_partial_kernel(const float* __restrict__ g, int64_t n4, const kzv_opt_group* __restrict__ groups,
                                                                    const int n_groups, float* __restrict__ partial) {
    __shared__ float red[4];
    float s = 0.f;
    GroupCursor c;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (int64_t)gridDim.x * 256) {
        c.seek(groups, n_groups, i * 4);
        if (c.lr_scale == 0.f) continue;
        const float4 v = ((const float4*)g)[i];
        s += v.x * v.x + v.y * v.y + v.z * v.z + v.w * v.w;
    }
    s = wave_sum(s);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) partial[blockIdx.x] = red[0] + red[1] + red[2] + red[3];
}

// clip_step_kernel with a group's scales: lr_t * lr_scale in both places lr_t enters (ylr and the z update), weight_decay * wd_scale.
// ckp1 is ONE value for all groups although schedulefree keeps lr_max and weight_sum per group: with r = 0 the weight of step k is
// lr_max_k ^ weight_lr_power, and a group whose learning rate is lr * lr_scale at every step has lr_max_k scaled by the same constant, so
// lr_scale ^ weight_lr_power multiplies the weight and every term of weight_sum alike and cancels in ckp1 = weight / weight_sum
// (tests/test_finetune_cpu.py pins this against the oracle's per-group state).  A frozen group (lr_scale == 0) is skipped whole: p, z, v
// and the EMA shadow are neither read nor written (v does not decay), and its gradient is outside *sqnorm (sqnorm_groups_partial_kernel),
// so the clip coefficient is the one of the trainable parameters.  Bytes per trainable parameter as in clip_step_kernel.
template <bool EMA>
__global__ __launch_bounds__(256) void clip_step_groups_kernel(float* __restrict__ p, float* __restrict__ z, float* __restrict__ v,
                                                               const float* __restrict__ g, int64_t n4,
                                                               const float* __restrict__ sqnorm, const kzv_opt_step s,
                                                               const kzv_opt_group* __restrict__ groups, const int n_groups,
                                                               float* __restrict__ ema, const float ema_w) {
    float gs = s.grad_scale;
    if (s.max_grad_norm > 0.f) {
        const float norm = sqrtf(*sqnorm) * fabsf(s.grad_scale);
        gs *= fminf(1.f, s.max_grad_norm / (norm + 1e-6f));
    }
    const float ylr1 = s.beta1 * (1.f - s.ckp1) - 1.f;
    const float inv_bc2 = 1.f / s.bias_correction2;
    GroupCursor c;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (int64_t)gridDim.x * 256) {
        c.seek(groups, n_groups, i * 4);
        if (c.lr_scale == 0.f) continue;
        const float lr = s.lr_t * c.lr_scale, ylr = lr * ylr1, wd = s.weight_decay * c.wd_scale;
        auto ntl = [](const float* q, int64_t i) { const f32x4 t = __builtin_nontemporal_load((const f32x4*)q + i); return make_float4(t[0], t[1], t[2], t[3]); };
        float4 P = ((float4*)p)[i], Z = ntl(z, i), V = ntl(v, i);
        const float4 G4 = ntl(g, i);
        float* pp = (float*)&P; float* zz = (float*)&Z; float* vv = (float*)&V; const float* gg = (const float*)&G4;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const float gr = gg[r] * gs;
            vv[r] = vv[r] * s.beta2 + s.one_minus_beta2 * gr * gr;
            float gn = s.adaptive ? gr / (sqrtf(vv[r] * inv_bc2) + s.eps) : gr;
            gn += wd * pp[r];
            float y = pp[r] + s.ckp1 * (zz[r] - pp[r]);
            y += ylr * gn;
            pp[r] = y;
            zz[r] -= lr * gn;
        }
        ((float4*)p)[i] = P;
        __builtin_nontemporal_store((f32x4){Z.x, Z.y, Z.z, Z.w}, (f32x4*)z + i); __builtin_nontemporal_store((f32x4){V.x, V.y, V.z, V.w}, (f32x4*)v + i);
        if (EMA) {
            float4 E = ((float4*)ema)[i];
            E.x += ema_w * (P.x - E.x); E.y += ema_w * (P.y - E.y); E.z += ema_w * (P.z - E.z); E.w += ema_w * (P.w - E.w);
            ((float4*)ema)[i] = E;
        }
    }
}

__global__ __launch_bounds__(256) void lerp_kernel(float* __restrict__ p, const float* __restrict__ z, int64_t n4, float w) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (int64_t)gridDim.x * 256) {
        float4 P = ((float4*)p)[i];
        const float4 Z = ((const float4*)z)[i];
        P.x += w * (Z.x - P.x); P.y += w * (Z.y - P.y); P.z += w * (Z.z - P.z); P.w += w * (Z.w - P.w);
        ((float4*)p)[i] = P;
    }
}

}  // namespace

int kzv_sqnorm(const float* g, int64_t n, float* out1, float* scratch, hipStream_t s) {
    if (n % 4) return kzv_fail(KZV_E_ARG, "sqnorm: n %% 4");
    hipLaunchKernelGGL(sqnorm_partial_kernel, dim3(NORM_BLOCKS), dim3(256), 0, s, g, n / 4, scratch);
    hipLaunchKernelGGL(sqnorm_final_kernel, dim3(1), dim3(256), 0, s, (const float*)scratch, NORM_BLOCKS, out1);
    return kzv_check_launch("sqnorm");
}

extern "C" int kzv_grad_sqnorm(const float* d_grads, int64_t n, float* d_out1, float* d_scratch, void* stream) {
    if (!d_grads || !d_out1 || !d_scratch) return kzv_fail(KZV_E_ARG, "grad_sqnorm: null");
    return kzv_sqnorm(d_grads, n, d_out1, d_scratch, (hipStream_t)stream);
}

extern "C" int kzv_clip_and_step_ema(float* d_params, float* d_z, float* d_v, const float* d_grads, int64_t n,
                                     const float* d_sqnorm, const kzv_opt_step* s, float* d_ema, float ema_decay, void* stream) {
    if (!d_params || !d_z || !d_v || !d_grads || !s) return kzv_fail(KZV_E_ARG, "clip_and_step: null");
    if (n % 4) return kzv_fail(KZV_E_ARG, "clip_and_step: n %% 4");
    if (s->max_grad_norm > 0.f && !d_sqnorm) return kzv_fail(KZV_E_ARG, "clip_and_step: clipping needs d_sqnorm");
    if (d_ema && !(ema_decay >= 0.f && ema_decay <= 1.f)) return kzv_fail(KZV_E_ARG, "clip_and_step: EMA decay must be in [0, 1]");
    if (d_ema) hipLaunchKernelGGL(clip_step_kernel<true>, dim3(2048), dim3(256), 0, (hipStream_t)stream, d_params, d_z, d_v, d_grads, n / 4, d_sqnorm, *s, d_ema, 1.f - ema_decay);
    else hipLaunchKernelGGL(clip_step_kernel<false>, dim3(2048), dim3(256), 0, (hipStream_t)stream, d_params, d_z, d_v, d_grads, n / 4, d_sqnorm, *s, (float*)nullptr, 0.f);
    return kzv_check_launch("clip_and_step");
}

extern "C" int kzv_clip_and_step(float* d_params, float* d_z, float* d_v, const float* d_grads, int64_t n,
                                 const float* d_sqnorm, const kzv_opt_step* s, void* stream) {
    return kzv_clip_and_step_ema(d_params, d_z, d_v, d_grads, n, d_sqnorm, s, nullptr, 0.f, stream);
}

// The table is device memory: what can be checked without reading it is checked here, its contents by the caller (kzv/optim.py:
// check_groups) before it is uploaded.
extern "C" int kzv_grad_sqnorm_groups(const float* d_grads, int64_t n, const kzv_opt_group* d_groups, int n_groups,
                                      float* d_out1, float* d_scratch, void* stream) {
    if (!d_grads || !d_groups || !d_out1 || !d_scratch) return kzv_fail(KZV_E_ARG, "grad_sqnorm_groups: null");
    if (n < 0 || n % 4) return kzv_fail(KZV_E_ARG, "grad_sqnorm_groups: n %% 4");
    if (n_groups < 1 || n_groups > KZV_OPT_MAX_GROUPS) return kzv_fail(KZV_E_ARG, "grad_sqnorm_groups: %d groups, 1..%d are served", n_groups, KZV_OPT_MAX_GROUPS);
    hipLaunchKernelGGL(sqnorm_groups_partial_kernel, dim3(NORM_BLOCKS), dim3(256), 0, (hipStream_t)stream, d_grads, n / 4, d_groups, n_groups, d_scratch);
    hipLaunchKernelGGL(sqnorm_final_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, (const float*)d_scratch, NORM_BLOCKS, d_out1);
    return kzv_check_launch("grad_sqnorm_groups");
}

extern "C" int kzv_clip_and_step_groups(float* d_params, float* d_z, float* d_v, const float* d_grads, int64_t n,
                                        const float* d_sqnorm, const kzv_opt_step* s, const kzv_opt_group* d_groups, int n_groups,
                                        float* d_ema, float ema_decay, void* stream) {
    if (!d_params || !d_z || !d_v || !d_grads || !s || !d_groups) return kzv_fail(KZV_E_ARG, "clip_and_step_groups: null");
    if (n < 0 || n % 4) return kzv_fail(KZV_E_ARG, "clip_and_step_groups: n %% 4");
    if (n_groups < 1 || n_groups > KZV_OPT_MAX_GROUPS) return kzv_fail(KZV_E_ARG, "clip_and_step_groups: %d groups, 1..%d are served", n_groups, KZV_OPT_MAX_GROUPS);
    if (s->max_grad_norm > 0.f && !d_sqnorm) return kzv_fail(KZV_E_ARG, "clip_and_step_groups: clipping needs d_sqnorm");
    if (d_ema && !(ema_decay >= 0.f && ema_decay <= 1.f)) return kzv_fail(KZV_E_ARG, "clip_and_step_groups: EMA decay must be in [0, 1]");
    if (d_ema) hipLaunchKernelGGL(clip_step_groups_kernel<true>, dim3(2048), dim3(256), 0, (hipStream_t)stream, d_params, d_z, d_v, d_grads, n / 4, d_sqnorm, *s, d_groups, n_groups, d_ema, 1.f - ema_decay);
    else hipLaunchKernelGGL(clip_step_groups_kernel<false>, dim3(2048), dim3(256), 0, (hipStream_t)stream, d_params, d_z, d_v, d_grads, n / 4, d_sqnorm, *s, d_groups, n_groups, (float*)nullptr, 0.f);
    return kzv_check_launch("clip_and_step_groups");
}

extern "C" int kzv_lerp_params(float* d_params, const float* d_z, int64_t n, float w, void* stream) {
    if (!d_params || !d_z || n % 4) return kzv_fail(KZV_E_ARG, "lerp_params: null or n %% 4");
    hipLaunchKernelGGL(lerp_kernel, dim3(2048), dim3(256), 0, (hipStream_t)stream, d_params, d_z, n / 4, w);
    return kzv_check_launch("lerp_params");
}
