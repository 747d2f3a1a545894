// d3m_morphable.h -- the vertices of a linear morphable model and the adjoint of that map (neural_renderer/morphable.py):
//
//   forward   out[b, r] = mean[r] + sum_k basis[r, k] * (scale[k] * coeffs[b, k])             basis [R, K] row-major f32
//   adjoint   grad_coeffs[b, k] = scale[k] * sum_r basis[r, k] * grad_out[b, r]
//
// Both stream the basis once per tile of MB_SETS coefficient sets and are HBM-bound passes.  f32 VALU, explicit fmaf (one
// rounding per term; the library's -ffp-contract=off concerns implicit contraction only).  No float atomics, no workgroup
// waits for another, every sum has a fixed order:
//
//   forward   a workgroup owns MB_FWD_ROWS rows, one per lane.  The basis tile goes through LDS in steps of MB_FWD_KC
//             components (coalesced 16-byte loads when K % 4 == 0 and the basis is 16-byte aligned, else 4-byte loads of
//             the same 256-byte runs; row stride MB_FWD_STRIDE words, so the lanes of a half wave read 32 distinct banks);
//             the scaled coefficients of the step are staged in LDS beside it.  Wave w adds components 16 w .. 16 w + 15
//             of every step in ascending order; the four waves' sums are added in wave order, then the mean.
//   adjoint   a workgroup owns the chunk of MB_ROWS consecutive rows blockIdx.x and the MB_KW components blockIdx.y; a lane
//             owns one component.  Wave w adds rows 64 w .. 64 w + 63 of the chunk in ascending order into one accumulator
//             per set (the chunk's grad_out values come from LDS, broadcast); the four waves' sums are added in wave order
//             and stored as partials[chunk, b, k].  k_morphable_adjoint_finish: group j of MB_FINISH_GROUPS adds the chunks
//             [j per, (j + 1) per), per = ceil(chunks / MB_FINISH_GROUPS), in ascending order; the groups' sums are added
//             in group order, then times scale[k] and grad_scale[b].
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace d3m {

constexpr int MB_SETS = 16;             // coefficient sets per pass over the basis
constexpr int MB_BLOCK = 256;
constexpr int MB_FWD_ROWS = 64;         // forward: rows per workgroup
constexpr int MB_FWD_KC = 64;           // forward: components per LDS step
constexpr int MB_FWD_STRIDE = MB_FWD_KC + 1;
constexpr int MB_ROWS = 256;            // adjoint: rows per chunk
constexpr int MB_WAVE_ROWS = 64;        // adjoint: rows per wave of a chunk
constexpr int MB_KW = 64;               // adjoint: components per workgroup
constexpr int MB_FINISH_GROUPS = 16;    // adjoint: groups of chunks in the finish
static_assert(MB_ROWS == 4 * MB_WAVE_ROWS && MB_BLOCK == 4 * 64 && MB_FWD_KC == 4 * 16, "four waves per workgroup");
static_assert(4 * MB_SETS * 64 <= MB_FWD_ROWS * MB_FWD_STRIDE, "the forward's wave sums reuse the tile");

// NB: the accumulators per lane, the smallest of 1, 4, 16 that holds the sets of a pass (sets beyond B are zeros, not stored)
template <int NB>
__global__ void __launch_bounds__(MB_BLOCK) k_morphable_forward(const float* __restrict__ basis, const float* __restrict__ coeffs,
                                                                const float* __restrict__ mean, const float* __restrict__ scale,
                                                                float* __restrict__ out, int B, int R, int K, int vec) {
    __shared__ float tile[MB_FWD_ROWS * MB_FWD_STRIDE];
    __shared__ __attribute__((aligned(16))) float sc[MB_FWD_KC * NB];       // [k][b]
    const int t = threadIdx.x, wave = t >> 6, lane = t & 63;
    const int r0 = blockIdx.x * MB_FWD_ROWS, b0 = blockIdx.y * MB_SETS;
    float acc[NB];
#pragma unroll
    for (int b = 0; b < NB; b++) acc[b] = 0.f;
    for (int kc = 0; kc < K; kc += MB_FWD_KC) {
        __syncthreads();                                    // the previous step's reads are done
        for (int i = t; i < MB_FWD_KC * NB; i += MB_BLOCK) {
            const int k = kc + i / NB, b = b0 + i % NB;
            float v = 0.f;
            if (k < K && b < B) {
                const float c = coeffs[(size_t)b * K + k];
                v = scale ? scale[k] * c : c;
            }
            sc[i] = v;
        }
        if (vec) {                                          // K % 4 == 0: a float4 lies inside its row or beyond it
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const int row = (t >> 4) + 16 * j, k4 = (t & 15) * 4, r = r0 + row, k = kc + k4;
                float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
                if (r < R && k < K) v = *reinterpret_cast<const float4*>(basis + (size_t)r * K + k);
                float* d = tile + row * MB_FWD_STRIDE + k4;
                d[0] = v.x; d[1] = v.y; d[2] = v.z; d[3] = v.w;
            }
        } else {
#pragma unroll 4
            for (int j = 0; j < 16; j++) {
                const int row = wave + 4 * j, r = r0 + row, k = kc + lane;
                tile[row * MB_FWD_STRIDE + lane] = (r < R && k < K) ? basis[(size_t)r * K + k] : 0.f;
            }
        }
        __syncthreads();
        const float* trow = tile + lane * MB_FWD_STRIDE + wave * 16;
        const float* s = sc + wave * 16 * NB;
#pragma unroll
        for (int i = 0; i < 16; i++) {
            const float x = trow[i];
#pragma unroll
            for (int b = 0; b < NB; b++) acc[b] = fmaf(x, s[i * NB + b], acc[b]);
        }
    }
    __syncthreads();
#pragma unroll
    for (int b = 0; b < NB; b++) tile[(wave * NB + b) * 64 + lane] = acc[b];
    __syncthreads();
    for (int i = t; i < NB * 64; i += MB_BLOCK) {
        const int b = i >> 6, row = i & 63, r = r0 + row;
        if (r < R && b0 + b < B) {
            float v = tile[b * 64 + row];
#pragma unroll
            for (int w = 1; w < 4; w++) v += tile[(w * NB + b) * 64 + row];
            out[(size_t)(b0 + b) * R + r] = mean ? mean[r] + v : v;
        }
    }
}

template <int NB>
__global__ void __launch_bounds__(MB_BLOCK) k_morphable_adjoint_chunks(const float* __restrict__ basis, const float* __restrict__ grad_out,
                                                                       float* __restrict__ partials, int B, int R, int K) {
    __shared__ __attribute__((aligned(16))) float g[NB * MB_ROWS];          // [b][row]; then the waves' sums [wave][b][lane]
    const int t = threadIdx.x, wave = t >> 6, lane = t & 63;
    const int chunk = blockIdx.x, r0 = chunk * MB_ROWS, k = blockIdx.y * MB_KW + lane, b0 = blockIdx.z * MB_SETS;
#pragma unroll
    for (int b = 0; b < NB; b++) {
        const int r = r0 + t;
        g[b * MB_ROWS + t] = (r < R && b0 + b < B) ? grad_out[(size_t)(b0 + b) * R + r] : 0.f;
    }
    __syncthreads();
    float acc[NB];
#pragma unroll
    for (int b = 0; b < NB; b++) acc[b] = 0.f;
    const bool active = k < K;
    const int wrow = wave * MB_WAVE_ROWS;
#pragma clang loop unroll_count(NB == 1 ? 2 : 1)        // 8 loads of the basis in flight per lane (16 with one set); more costs occupancy
    for (int rr = 0; rr < MB_WAVE_ROWS; rr += 8) {
        float x[8];
#pragma unroll
        for (int j = 0; j < 8; j++) {
            const int r = r0 + wrow + rr + j;
            x[j] = (active && r < R) ? basis[(size_t)r * K + k] : 0.f;
        }
#pragma unroll
        for (int b = 0; b < NB; b++) {
            const float4 g0 = *reinterpret_cast<const float4*>(g + b * MB_ROWS + wrow + rr);
            const float4 g1 = *reinterpret_cast<const float4*>(g + b * MB_ROWS + wrow + rr + 4);
            float a = acc[b];
            a = fmaf(x[0], g0.x, a); a = fmaf(x[1], g0.y, a); a = fmaf(x[2], g0.z, a); a = fmaf(x[3], g0.w, a);
            a = fmaf(x[4], g1.x, a); a = fmaf(x[5], g1.y, a); a = fmaf(x[6], g1.z, a); a = fmaf(x[7], g1.w, a);
            acc[b] = a;
        }
    }
    __syncthreads();
#pragma unroll
    for (int b = 0; b < NB; b++) g[(wave * NB + b) * 64 + lane] = acc[b];
    __syncthreads();
    for (int i = t; i < NB * 64; i += MB_BLOCK) {
        const int b = i >> 6, l = i & 63, kk = blockIdx.y * MB_KW + l;
        if (kk < K && b0 + b < B) {
            float v = g[b * 64 + l];
#pragma unroll
            for (int w = 1; w < 4; w++) v += g[(w * NB + b) * 64 + l];
            partials[((size_t)chunk * B + b0 + b) * K + kk] = v;
        }
    }
}

__global__ void __launch_bounds__(MB_FINISH_GROUPS * 64) k_morphable_adjoint_finish(const float* __restrict__ partials, int n_chunks,
                                                                                   const float* __restrict__ scale,
                                                                                   const float* __restrict__ grad_scale,
                                                                                   float* __restrict__ grad_coeffs, int B, int K,
                                                                                   int accumulate) {
    __shared__ float group_sum[MB_FINISH_GROUPS * 64];
    const int lane = threadIdx.x & 63, group = threadIdx.x >> 6, k = blockIdx.x * 64 + lane, b = blockIdx.y;
    const int per = (n_chunks + MB_FINISH_GROUPS - 1) / MB_FINISH_GROUPS;
    const int c0 = group * per, c1 = min(c0 + per, n_chunks);
    float s = 0.f;
    if (k < K) {
#pragma unroll 8
        for (int c = c0; c < c1; c++) s += partials[((size_t)c * B + b) * K + k];
    }
    group_sum[group * 64 + lane] = s;
    __syncthreads();
    if (group == 0 && k < K) {
        float v = group_sum[lane];
#pragma unroll
        for (int j = 1; j < MB_FINISH_GROUPS; j++) v += group_sum[j * 64 + lane];
        if (scale) v = scale[k] * v;
        if (grad_scale) v = grad_scale[b] * v;
        float* dst = grad_coeffs + (size_t)b * K + k;
        *dst = accumulate ? *dst + v : v;
    }
}

}  // namespace d3m
