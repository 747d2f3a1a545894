// d3m_uv_texture_reg.h -- regularisers of a UV texture x [B, H, W, C] (channels last, row j = texture row j), 1 <= C <= 4:
// smoothness, left-right symmetry, flatness and an anchor to a reference texture, value and gradient, per image b
// (neural_renderer/uv_texture_regularizers.py).  A texel is ACTIVE iff its mask value is > 0 (negative and NaN: absent; no
// mask: every texel).  With t = (i, j) a texel, k a channel:
//
//   smooth   S_s = sum over the active texels t of  [j + 1 < W, (i, j + 1) active] sum_k rho(x_t[k] - x_(i,j+1)[k])
//                                                 + [i + 1 < H, (i + 1, j) active] sum_k rho(x_t[k] - x_(i+1,j)[k])
//            (a pair is counted at its upper / left texel; P = the pairs), rho(d) = d^2 without eps and
//            d^2 / (sqrt(d^2 + eps^2) + eps) with it: sqrt(d^2 + eps^2) - eps without the cancellation, exactly +0 at d = 0;
//            rho'(d) = 2 d and d / sqrt(d^2 + eps^2)
//   symmetry S_y = sum over the active t with j < W - 1 - j whose mirror texel m = (i, W - 1 - j) is active of
//            sum_k (x_t[k] - x_m[k])^2      (M = these texels)
//   flat     S_f = sum over the active t of sum_k (x_t[k] - mu_k)^2,  mu_k = (sum over the active t of x_t[k]) / N  (N = the
//            active texels)
//   anchor   S_a = sum over the active t of r_t sum_k (x_t[k] - ref_t[k])^2,  r_t = the reference weight where it is > 0, else
//            0 (no weights: 1);  R = sum over the active t of r_t
//
//   value[b] = ((c_s S_s + c_y S_y) + c_f S_f) + c_a S_a over the terms of weight > 0, in this order, from the first one;
//              c_s = smooth / (P C), c_y = symmetry / (M C), c_f = flat / (N C), c_a = anchor / (R C), each formed in f64 and
//              rounded to f32 once; a term whose count is 0 has c = 0 and adds exactly +0
//   grad[t, k] = scale[b] (((c_s (rho'(x_t - x_left) + rho'(x_t - x_right) + rho'(x_t - x_up) + rho'(x_t - x_down))
//                + c_y 2 (x_t - x_m)) + c_f 2 (x_t - mu)) + c_a 2 r_t (x_t - ref_t)),  the neighbours that are active, in this
//                order, from +0; an inactive texel and every texel of an image with scale[b] == 0 get exactly +0.
//
// The gradient is a gather: a lane owns a texel, reads its up-to-four neighbours and its mirror texel from global memory
// and stores its C values once.  No float atomics, nothing cleared, every element written.
//
// Passes (d3m_set_sums.h states the tree; UVR_PER_PART texels per part, at most UVR_MAX_PARTS parts per image, DppRows):
//   k_uv_texture_reg_stats         grid (parts, B): the float sums R and sum_t x_t[k] (5 per part), and the counts P, M, N as
//                                  integers: a lane counts in an int, the wave and the four waves add ints (exact in any
//                                  order), stored beside the float partials
//   k_uv_texture_reg_stats_finish  a workgroup per image stages the parts in LDS; lane 0 adds them in ascending order (the
//                                  counts in 64 bits) and leaves stats [B, 4 + C] = (c_s, c_y, c_f, c_a, mu[C])
//   k_uv_texture_reg_terms         grid (parts, B): the four value sums per part (when the value is wanted) and the
//                                  gradient of every texel (when it is)
//   k_uv_texture_reg_value_finish  likewise: lane 0 adds the image's parts in ascending order and forms value[b]
// The counts are computed on the device on every call: a mask may change every step, and nothing here synchronises.
#pragma once
#include "d3m_aux.h"
#include "d3m_set_sums.h"

namespace d3m {

constexpr int UVR_MAX_CHANNELS = 4;
constexpr int UVR_PER_PART = SET_BLOCK;     // texels per part: one per lane
constexpr int UVR_MAX_PARTS = 256;          // workgroups per image; beyond UVR_PER_PART * UVR_MAX_PARTS texels the lanes stride
constexpr int UVR_STAT_SUMS = 1 + UVR_MAX_CHANNELS;      // R, sum x[k]
constexpr int UVR_COUNTS = 4;               // P, M, N (and a word of padding)
constexpr int UVR_VALUE_SUMS = 4;           // S_s, S_y, S_f, S_a
constexpr int UVR_STATS = 4;                // c_s, c_y, c_f, c_a; mu[C] follows
constexpr float UVR_NO_EPS = -1.0f;         // smooth_eps of the squared difference

__host__ __device__ __forceinline__ int uvr_parts(long texels) { return set_parts(texels, UVR_PER_PART, UVR_MAX_PARTS); }

struct UvTextureReg {
    const float* x;             // [B, H, W, C]
    const float* mask;          // [mask_batch, H, W] or NULL (every texel active)
    const float* ref;           // [ref_batch, H, W, C]; read only with w_anchor > 0
    const float* ref_weights;   // [rw_batch, H, W] or NULL (1)
    int B, H, W, mask_batch, ref_batch, rw_batch;
    float w_smooth, w_sym, w_flat, w_anchor;        // 0: the term is off
    float eps;                  // UVR_NO_EPS: rho(d) = d^2
};

__device__ __forceinline__ bool uvr_active(const float* __restrict__ mask, int t) { return !mask || mask[t] > 0.f; }

template <int C>
__device__ __forceinline__ void uvr_load(const float* __restrict__ x, int t, float (&v)[C]) {
    const float* p = x + (size_t)t * C;
    if constexpr (C == 4) {
        const float4 q = *reinterpret_cast<const float4*>(p);           // (C floats are C * 4 bytes aligned: the entry points check)
        v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
    } else if constexpr (C == 2) {
        const float2 q = *reinterpret_cast<const float2*>(p);
        v[0] = q.x; v[1] = q.y;
    } else {
#pragma unroll
        for (int k = 0; k < C; k++) v[k] = p[k];
    }
}

template <int C>
__device__ __forceinline__ void uvr_store(float* __restrict__ x, int t, const float (&v)[C]) {
    float* p = x + (size_t)t * C;
    if constexpr (C == 4) {
        *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
    } else if constexpr (C == 2) {
        *reinterpret_cast<float2*>(p) = make_float2(v[0], v[1]);
    } else {
#pragma unroll
        for (int k = 0; k < C; k++) p[k] = v[k];
    }
}

// the image's planes
__device__ __forceinline__ const float* uvr_plane(const float* p, int batch, int b, size_t n) {
    return p ? p + (size_t)(batch > 1 ? b : 0) * n : nullptr;
}

// ---- the counts and the sums behind mu and R ----------------------------------------------------------------------------------
template <int C>
__global__ void __launch_bounds__(SET_BLOCK) k_uv_texture_reg_stats(UvTextureReg a, float* __restrict__ partial,
                                                                    int* __restrict__ count_partial) {
    __shared__ float s_wave[4][UVR_STAT_SUMS];
    __shared__ int s_count[4][UVR_COUNTS];
    const int b = blockIdx.y, parts = gridDim.x, H = a.H, W = a.W, n = H * W;
    const float* x = a.x + (size_t)b * n * C;
    const float* mask = uvr_plane(a.mask, a.mask_batch, b, n);
    const float* rw = uvr_plane(a.ref_weights, a.rw_batch, b, n);
    float acc[UVR_STAT_SUMS];
#pragma unroll
    for (int k = 0; k < UVR_STAT_SUMS; k++) acc[k] = 0.f;
    int cnt[3] = {0, 0, 0};
    for (int t = blockIdx.x * SET_BLOCK + threadIdx.x; t < n; t += parts * SET_BLOCK) {
        if (!uvr_active(mask, t)) continue;
        cnt[2]++;
        const int i = t / W, j = t - i * W;
        if (a.w_smooth > 0.f) {
            if (j + 1 < W && uvr_active(mask, t + 1)) cnt[0]++;
            if (i + 1 < H && uvr_active(mask, t + W)) cnt[0]++;
        }
        if (a.w_sym > 0.f && j < W - 1 - j && uvr_active(mask, t + (W - 1 - 2 * j))) cnt[1]++;
        if (a.w_anchor > 0.f) {
            const float r = rw ? rw[t] : 1.f;
            acc[0] += r > 0.f ? r : 0.f;
        }
        if (a.w_flat > 0.f) {
            float v[C];
            uvr_load<C>(x, t, v);
#pragma unroll
            for (int k = 0; k < C; k++) acc[1 + k] += v[k];
        }
    }
#pragma unroll
    for (int k = 0; k < 3; k++) {
        for (int off = 32; off >= 1; off >>= 1) cnt[k] += __shfl_xor(cnt[k], off, 64);
    }
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int k = 0; k < 3; k++) s_count[threadIdx.x >> 6][k] = cnt[k];
    }
    set_store_partial<UVR_STAT_SUMS, WaveTree::DppRows>(acc, s_wave, partial, b, parts);       // (its barrier covers s_count)
    if (threadIdx.x < UVR_COUNTS) {
        const int k = threadIdx.x;
        count_partial[((size_t)b * parts + blockIdx.x) * UVR_COUNTS + k] =
            k < 3 ? s_count[0][k] + s_count[1][k] + s_count[2][k] + s_count[3][k] : 0;
    }
}

// weight / (count C), in f64, rounded once; 0 for a count of 0
__device__ __forceinline__ float uvr_coefficient(float weight, double count, int C) {
    return weight > 0.f && count > 0.0 ? (float)((double)weight / (count * (double)C)) : 0.f;
}

// One workgroup per image: the lanes stage the image's parts in LDS (a lane that walked them in global memory waited for
// every part in turn), then lane 0 adds them in ascending order.
__global__ void __launch_bounds__(SET_BLOCK) k_uv_texture_reg_stats_finish(UvTextureReg a, int C, const float* __restrict__ partial,
                                                                           const int* __restrict__ count_partial, int parts,
                                                                           float* __restrict__ stats) {
    __shared__ float s_part[UVR_MAX_PARTS * UVR_STAT_SUMS];
    __shared__ int s_count[UVR_MAX_PARTS * UVR_COUNTS];
    const int b = blockIdx.x;
    for (int i = threadIdx.x; i < parts * UVR_STAT_SUMS; i += SET_BLOCK) s_part[i] = partial[(size_t)b * parts * UVR_STAT_SUMS + i];
    for (int i = threadIdx.x; i < parts * UVR_COUNTS; i += SET_BLOCK) s_count[i] = count_partial[(size_t)b * parts * UVR_COUNTS + i];
    __syncthreads();
    if (threadIdx.x != 0) return;
    float s[UVR_STAT_SUMS];
    set_add_parts(s_part, 0, parts, s);
    long long cnt[3] = {0, 0, 0};
    for (int p = 0; p < parts; p++) {
#pragma unroll
        for (int k = 0; k < 3; k++) cnt[k] += s_count[p * UVR_COUNTS + k];
    }
    float* o = stats + (size_t)b * (UVR_STATS + C);
    o[0] = uvr_coefficient(a.w_smooth, (double)cnt[0], C);
    o[1] = uvr_coefficient(a.w_sym, (double)cnt[1], C);
    o[2] = uvr_coefficient(a.w_flat, (double)cnt[2], C);
    o[3] = uvr_coefficient(a.w_anchor, cnt[2] > 0 ? (double)s[0] : 0.0, C);
    const float n = (float)cnt[2];
    for (int k = 0; k < C; k++) o[UVR_STATS + k] = a.w_flat > 0.f && cnt[2] > 0 ? s[1 + k] / n : 0.f;
}

// ---- the terms: value partials and the gathered gradient ------------------------------------------------------------------------
template <bool CHARBONNIER>
__device__ __forceinline__ float uvr_rho(float d, float eps) {
    if constexpr (CHARBONNIER) return (d * d) / (sqrtf(d * d + eps * eps) + eps);
    else return d * d;
}
template <bool CHARBONNIER>
__device__ __forceinline__ float uvr_rho_slope(float d, float eps) {
    if constexpr (CHARBONNIER) return d / sqrtf(d * d + eps * eps);
    else return 2.0f * d;
}

// value_partial [B, parts, UVR_VALUE_SUMS] or NULL (the value is not wanted); grad [B, H, W, C] or NULL; grad_scale [B] or
// NULL (1); stats [B, UVR_STATS + C].
template <int C, bool CHARBONNIER>
__global__ void __launch_bounds__(SET_BLOCK) k_uv_texture_reg_terms(UvTextureReg a, const float* __restrict__ stats,
                                                                    const float* __restrict__ grad_scale,
                                                                    float* __restrict__ value_partial, float* __restrict__ grad) {
    __shared__ float s_wave[4][UVR_VALUE_SUMS];
    const int b = blockIdx.y, parts = gridDim.x, H = a.H, W = a.W, n = H * W;
    const float* x = a.x + (size_t)b * n * C;
    const float* mask = uvr_plane(a.mask, a.mask_batch, b, n);
    const float* rw = uvr_plane(a.ref_weights, a.rw_batch, b, n);
    const float* ref = uvr_plane(a.ref, a.ref_batch, b, (size_t)n * C);
    const float* st = stats + (size_t)b * (UVR_STATS + C);
    // (a term that is off reads none of its inputs, whatever the statistics say)
    const float c_s = a.w_smooth > 0.f ? st[0] : 0.f, c_y = a.w_sym > 0.f ? st[1] : 0.f, c_f = a.w_flat > 0.f ? st[2] : 0.f,
                c_a = a.w_anchor > 0.f ? st[3] : 0.f;
    float mu[C];
#pragma unroll
    for (int k = 0; k < C; k++) mu[k] = st[UVR_STATS + k];
    const float scale = grad_scale ? grad_scale[b] : 1.f;
    const bool want_grad = grad != nullptr, live = want_grad && scale != 0.f;       // (uniform over the workgroup)
    float* g_out = want_grad ? grad + (size_t)b * n * C : nullptr;
    const float eps = a.eps;
    float acc[UVR_VALUE_SUMS] = {0.f, 0.f, 0.f, 0.f};
    for (int t = blockIdx.x * SET_BLOCK + threadIdx.x; t < n; t += parts * SET_BLOCK) {
        float g[C];
#pragma unroll
        for (int k = 0; k < C; k++) g[k] = 0.f;
        if ((value_partial || live) && uvr_active(mask, t)) {
            const int i = t / W, j = t - i * W;
            float v[C], u[C];
            uvr_load<C>(x, t, v);
            if (c_s > 0.f) {
                float slope[C];
#pragma unroll
                for (int k = 0; k < C; k++) slope[k] = 0.f;
                if (live && j > 0 && uvr_active(mask, t - 1)) {
                    uvr_load<C>(x, t - 1, u);
#pragma unroll
                    for (int k = 0; k < C; k++) slope[k] += uvr_rho_slope<CHARBONNIER>(v[k] - u[k], eps);
                }
                if (j + 1 < W && uvr_active(mask, t + 1)) {
                    uvr_load<C>(x, t + 1, u);
#pragma unroll
                    for (int k = 0; k < C; k++) {
                        const float d = v[k] - u[k];
                        slope[k] += uvr_rho_slope<CHARBONNIER>(d, eps);
                        acc[0] += uvr_rho<CHARBONNIER>(d, eps);
                    }
                }
                if (live && i > 0 && uvr_active(mask, t - W)) {
                    uvr_load<C>(x, t - W, u);
#pragma unroll
                    for (int k = 0; k < C; k++) slope[k] += uvr_rho_slope<CHARBONNIER>(v[k] - u[k], eps);
                }
                if (i + 1 < H && uvr_active(mask, t + W)) {
                    uvr_load<C>(x, t + W, u);
#pragma unroll
                    for (int k = 0; k < C; k++) {
                        const float d = v[k] - u[k];
                        slope[k] += uvr_rho_slope<CHARBONNIER>(d, eps);
                        acc[0] += uvr_rho<CHARBONNIER>(d, eps);
                    }
                }
#pragma unroll
                for (int k = 0; k < C; k++) g[k] = c_s * slope[k];
            }
            if (c_y > 0.f) {
                const int jm = W - 1 - j;
                if (jm != j && uvr_active(mask, t + (jm - j))) {
                    uvr_load<C>(x, t + (jm - j), u);
#pragma unroll
                    for (int k = 0; k < C; k++) {
                        const float d = v[k] - u[k];
                        g[k] += c_y * (2.0f * d);
                        if (j < jm) acc[1] += d * d;
                    }
                }
            }
            if (c_f > 0.f) {
#pragma unroll
                for (int k = 0; k < C; k++) {
                    const float d = v[k] - mu[k];
                    g[k] += c_f * (2.0f * d);
                    acc[2] += d * d;
                }
            }
            if (c_a > 0.f) {
                float r = rw ? rw[t] : 1.f;
                r = r > 0.f ? r : 0.f;
                if (r > 0.f) {
                    uvr_load<C>(ref, t, u);
#pragma unroll
                    for (int k = 0; k < C; k++) {
                        const float d = v[k] - u[k];
                        g[k] += c_a * (2.0f * (r * d));
                        acc[3] += r * (d * d);
                    }
                }
            }
        }
        if (want_grad) {
#pragma unroll
            for (int k = 0; k < C; k++) g[k] = live ? scale * g[k] + 0.f : 0.f;          // (-0 + +0 is +0)
            uvr_store<C>(g_out, t, g);
        }
    }
    if (value_partial)                                      // (uniform: the barrier is met by every lane)
        set_store_partial<UVR_VALUE_SUMS, WaveTree::DppRows>(acc, s_wave, value_partial, b, parts);
}

__global__ void __launch_bounds__(SET_BLOCK) k_uv_texture_reg_value_finish(UvTextureReg a, int C, const float* __restrict__ stats,
                                                                           const float* __restrict__ value_partial, int parts,
                                                                           float* __restrict__ value) {
    __shared__ float s_part[UVR_MAX_PARTS * UVR_VALUE_SUMS];
    const int b = blockIdx.x;
    for (int i = threadIdx.x; i < parts * UVR_VALUE_SUMS; i += SET_BLOCK)
        s_part[i] = value_partial[(size_t)b * parts * UVR_VALUE_SUMS + i];
    __syncthreads();
    if (threadIdx.x != 0) return;
    float s[UVR_VALUE_SUMS];
    set_add_parts(s_part, 0, parts, s);
    const float* st = stats + (size_t)b * (UVR_STATS + C);
    const float w[4] = {a.w_smooth, a.w_sym, a.w_flat, a.w_anchor};
    float total = 0.f;
    bool first = true;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        if (!(w[k] > 0.f)) continue;
        const float term = st[k] > 0.f ? st[k] * s[k] : 0.f;
        total = first ? term : total + term;
        first = false;
    }
    value[b] = total;
}

}  // namespace d3m
