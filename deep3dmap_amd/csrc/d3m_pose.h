// d3m_pose.h -- the weak-perspective pose of a point set and its adjoint (neural_renderer/pose.py):
//
//   a        = clamp(pose[b, 1:4], -limit, +limit)              R_b = Rx(a0) Ry(a1) Rz(a2), the factors of euler_factors
//   posed[b, v] = s_b (R_b x[v]) + tau t_b                       s_b = pose[b, 0], t_b = pose[b, 4:7]
//   uv[b, v]    = (posed_x / uv_size, 1 - posed_y / uv_size)
//   lm[b, l]    = posed[b, landmarks[l]]
//
// and, with G[b, v] = g_posed + (g_uv.x / uv_size, -g_uv.y / uv_size, 0) + the landmark gradients that point at v,
//
//   M_b = sum_v G (x) x   n_b = sum_v G      g_s = <M_b, R_b>   g_a_k = s_b <M_b, dR_b/da_k> [|pose[b, 1 + k]| <= limit]
//   g_t = tau n_b                            g_x[b, v] = s_b R_b^T G[b, v]   (shared vertices: summed over b, ascending)
//
// Plain f32 VALU streaming; the library's -ffp-contract=off rounds every operation once.  R_b is computed once per
// workgroup by a prologue lane (pose_stage), never per vertex.  No float atomics, no workgroup waits for another, every
// sum has a fixed order:
//
//   k_pose_forward          grid (parts, B): lanes stride over the V vertices, then over the L landmarks (the same
//                           expression on the gathered point, so lm equals the rows of posed bit for bit).
//   k_pose_backward_chunks  grid (parts, B), or (parts, 1) with shared vertices, where the workgroup walks the sets in
//                           ascending order and adds into its own g_x elements.  The 12 sums (M row-major, then n) of a
//                           set: WaveTree::DppRows, PS_BLOCK vertices per part up to PS_MAX_PARTS parts, see
//                           d3m_set_sums.h.  g_x is written from the same read of G.
//   k_pose_backward_finish  a lane per set adds the set's partials (d3m_set_sums.h, step 4), then the landmark terms in
//                           ascending l, and applies the Euler adjoint.  Further workgroups of the same launch add the
//                           landmark gradients to g_x: per-set vertices, a lane per (set, coordinate) that walks l in
//                           ascending order; shared vertices, one workgroup that first sums every (l, coordinate) over the
//                           sets in ascending order in LDS, then three lanes walk l in ascending order.
#pragma once
#include "d3m_aux.h"
#include "d3m_set_sums.h"

namespace d3m {

constexpr int PS_BLOCK = 256;           // lanes of a forward / chunk workgroup: the vertices of one chunk
constexpr int PS_MAX_PARTS = 64;        // workgroups per set; beyond PS_BLOCK * PS_MAX_PARTS vertices the lanes stride
constexpr int PS_SUMS = 12;             // M_b (9, row-major) and n_b (3)
constexpr int PS_FINISH_SETS = 64;      // sets per finish workgroup, one per lane
constexpr int PS_STAGE = 64;            // rotations staged in LDS at a time
constexpr int PS_ROT = 13;              // R (9), s, tau t (3)
constexpr int PS_MAX_LANDMARKS = 1024;

__host__ __device__ __forceinline__ int pose_parts(long items) { return set_parts(items, PS_BLOCK, PS_MAX_PARTS); }

// the clamped angles' factors
__device__ __forceinline__ void pose_factors(const float* p, float limit, float* mx, float* my, float* mz, float* cs) {
    float a[3];
#pragma unroll
    for (int k = 0; k < 3; k++) a[k] = limit > 0.f ? fminf(fmaxf(p[1 + k], -limit), limit) : p[1 + k];
#pragma unroll
    for (int k = 0; k < 3; k++) { cs[2 * k] = cosf(a[k]); cs[2 * k + 1] = sinf(a[k]); }
    euler_factors(cs[0], cs[1], cs[2], cs[3], cs[4], cs[5], mx, my, mz);
}

// rot[0..8] = R = (Rx Ry) Rz, rot[9] = s, rot[10..12] = tau t
__device__ __forceinline__ void pose_stage(const float* p, float tau, float limit, float* rot) {
    float mx[9], my[9], mz[9], cs[6], xy[9], r[9];
    pose_factors(p, limit, mx, my, mz, cs);
    mat3_mul(mx, my, xy);
    mat3_mul(xy, mz, r);
#pragma unroll
    for (int k = 0; k < 9; k++) rot[k] = r[k];
    rot[9] = p[0];
#pragma unroll
    for (int k = 0; k < 3; k++) rot[10 + k] = tau * p[4 + k];
}

// s R^T g, component j
__device__ __forceinline__ float pose_pull(const float* r, float s, const float* g, int j) {
    return s * ((r[j] * g[0] + r[3 + j] * g[1]) + r[6 + j] * g[2]);
}

__global__ void __launch_bounds__(PS_BLOCK) k_pose_forward(const float* __restrict__ vertices, int vb,
                                                           const float* __restrict__ pose, int pose_stride, float tau,
                                                           float limit, float uv_size,
                                                           const int32_t* __restrict__ landmarks, int L,
                                                           float* __restrict__ posed, float* __restrict__ uv,
                                                           float* __restrict__ lm, int V) {
    __shared__ float s_rot[PS_ROT];
    const int b = blockIdx.y;
    if (threadIdx.x == 0) pose_stage(pose + (size_t)b * pose_stride, tau, limit, s_rot);
    __syncthreads();
    float r[PS_ROT];
#pragma unroll
    for (int k = 0; k < PS_ROT; k++) r[k] = s_rot[k];
    const float* x0 = vertices + (size_t)(vb > 1 ? b : 0) * V * 3;
    const int nv = (posed || uv) ? V : 0, items = nv + (lm ? L : 0);
    for (int i = blockIdx.x * PS_BLOCK + threadIdx.x; i < items; i += gridDim.x * PS_BLOCK) {
        const int v = i < nv ? i : landmarks[i - nv];
        const float* x = x0 + (size_t)v * 3;
        const float x_[3] = {x[0], x[1], x[2]};
        float p[3];
#pragma unroll
        for (int j = 0; j < 3; j++)
            p[j] = r[9] * ((r[3 * j] * x_[0] + r[3 * j + 1] * x_[1]) + r[3 * j + 2] * x_[2]) + r[10 + j];
        if (i < nv) {
            const size_t at = (size_t)b * V + i;
            if (posed) { posed[at * 3] = p[0]; posed[at * 3 + 1] = p[1]; posed[at * 3 + 2] = p[2]; }
            if (uv) { uv[at * 2] = p[0] / uv_size; uv[at * 2 + 1] = 1.f - p[1] / uv_size; }
        } else {
            float* d = lm + ((size_t)b * L + (i - nv)) * 3;
            d[0] = p[0]; d[1] = p[1]; d[2] = p[2];
        }
    }
}

// grid (parts, B) with per-set vertices (vb > 1), (parts, 1) with shared ones.  partial [B, parts, PS_SUMS] or NULL;
// g_x [vb > 1 ? B : 1, V, 3] or NULL; g_posed / g_uv may be NULL (zeros).
__global__ void __launch_bounds__(PS_BLOCK) k_pose_backward_chunks(const float* __restrict__ vertices, int vb,
                                                                   const float* __restrict__ pose, int pose_stride,
                                                                   float limit, float uv_size,
                                                                   const float* __restrict__ g_posed,
                                                                   const float* __restrict__ g_uv, float* g_x,
                                                                   float* __restrict__ partial, int B, int V) {
    __shared__ float s_rot[PS_STAGE][PS_ROT];
    __shared__ float s_wave[2][4][PS_SUMS];
    const int t = threadIdx.x, parts = gridDim.x;
    const bool shared = vb <= 1;
    const int b_begin = shared ? 0 : blockIdx.y, b_end = shared ? B : b_begin + 1;
    for (int b0 = b_begin; b0 < b_end; b0 += PS_STAGE) {
        const int n = min(PS_STAGE, b_end - b0);
        __syncthreads();                                    // the previous stage's reads are done
        if (t < n) pose_stage(pose + (size_t)(b0 + t) * pose_stride, 0.f, limit, s_rot[t]);
        __syncthreads();
        for (int k = 0; k < n; k++) {
            const int b = b0 + k;
            float r[9];
#pragma unroll
            for (int j = 0; j < 9; j++) r[j] = s_rot[k][j];
            const float s = s_rot[k][9];
            float acc[PS_SUMS];
#pragma unroll
            for (int j = 0; j < PS_SUMS; j++) acc[j] = 0.f;
            for (int i = blockIdx.x * PS_BLOCK + t; i < V; i += parts * PS_BLOCK) {
                const size_t at = (size_t)b * V + i;
                float g[3] = {0.f, 0.f, 0.f};
                if (g_posed) { g[0] = g_posed[at * 3]; g[1] = g_posed[at * 3 + 1]; g[2] = g_posed[at * 3 + 2]; }
                if (g_uv) { g[0] += g_uv[at * 2] / uv_size; g[1] -= g_uv[at * 2 + 1] / uv_size; }
                const size_t xat = ((size_t)(shared ? 0 : b) * V + i) * 3;
                if (partial) {
                    const float x[3] = {vertices[xat], vertices[xat + 1], vertices[xat + 2]};
#pragma unroll
                    for (int j = 0; j < 3; j++) {
#pragma unroll
                        for (int c = 0; c < 3; c++) acc[3 * j + c] += g[j] * x[c];
                        acc[9 + j] += g[j];
                    }
                }
                if (g_x) {
#pragma unroll
                    for (int j = 0; j < 3; j++) {
                        const float v = pose_pull(r, s, g, j);
                        g_x[xat + j] = b > b_begin ? g_x[xat + j] + v : v;      // (this lane's own element)
                    }
                }
            }
            if (partial)                                    // (uniform: the barrier is met by every lane)
                set_store_partial<PS_SUMS, WaveTree::DppRows>(      // two buffers: set k + 1 is written while set k is read
                    acc, s_wave[k & 1], partial, b, parts);
        }
    }
}

// grid (pose_blocks + landmark blocks), PS_FINISH_SETS lanes.  Workgroups below pose_blocks: g_pose [B, 7] from the
// partials (parts may be 0) and the landmark terms.  The others (present when g_lm and g_x are given): g_x += the
// landmark gradients.
__global__ void __launch_bounds__(PS_FINISH_SETS) k_pose_backward_finish(const float* __restrict__ vertices, int vb,
                                                                        const float* __restrict__ pose, int pose_stride,
                                                                        float tau, float limit,
                                                                        const int32_t* __restrict__ landmarks, int L,
                                                                        const float* __restrict__ g_lm,
                                                                        const float* __restrict__ partial, int parts,
                                                                        float* g_x, float* __restrict__ g_pose, int B, int V,
                                                                        int pose_blocks) {
    __shared__ float s_rot[PS_STAGE][PS_ROT];
    __shared__ float s_h[3 * PS_MAX_LANDMARKS];
    const int t = threadIdx.x;
    if ((int)blockIdx.x < pose_blocks) {
        const int b = blockIdx.x * PS_FINISH_SETS + t;
        if (b >= B) return;
        float m[PS_SUMS];
        set_add_parts(partial, b, parts, m);
        if (g_lm) {
            const float* x0 = vertices + (size_t)(vb > 1 ? b : 0) * V * 3;
            for (int l = 0; l < L; l++) {
                const float* g = g_lm + ((size_t)b * L + l) * 3;
                const float* x = x0 + (size_t)landmarks[l] * 3;
#pragma unroll
                for (int j = 0; j < 3; j++) {
#pragma unroll
                    for (int c = 0; c < 3; c++) m[3 * j + c] += g[j] * x[c];
                    m[9 + j] += g[j];
                }
            }
        }
        const float* p = pose + (size_t)b * pose_stride;
        float mx[9], my[9], mz[9], cs[6], t0[9], t1[9];
        pose_factors(p, limit, mx, my, mz, cs);
        // derivatives of the factors: d/dtheta of (cos, sin) = (-sin, cos), constants -> 0
        const float dx[9] = {0, 0, 0, 0, -cs[1], -cs[0], 0, cs[0], -cs[1]};
        const float dy[9] = {-cs[3], 0, cs[2], 0, 0, 0, -cs[2], 0, -cs[3]};
        const float dz[9] = {-cs[5], -cs[4], 0, cs[4], -cs[5], 0, 0, 0, 0};
        float out[4];
        mat3_mul(mx, my, t0); mat3_mul(t0, mz, t1);          // R = (Rx Ry) Rz
        out[0] = 0; for (int k = 0; k < 9; k++) out[0] += m[k] * t1[k];
        mat3_mul(dx, my, t0); mat3_mul(t0, mz, t1);          // dR/da0 = (Rx' Ry) Rz
        out[1] = 0; for (int k = 0; k < 9; k++) out[1] += m[k] * t1[k];
        mat3_mul(mx, dy, t0); mat3_mul(t0, mz, t1);          // dR/da1 = (Rx Ry') Rz
        out[2] = 0; for (int k = 0; k < 9; k++) out[2] += m[k] * t1[k];
        mat3_mul(mx, my, t0); mat3_mul(t0, dz, t1);          // dR/da2 = (Rx Ry) Rz'
        out[3] = 0; for (int k = 0; k < 9; k++) out[3] += m[k] * t1[k];
        float* o = g_pose + (size_t)b * 7;
        o[0] = out[0];
#pragma unroll
        for (int k = 0; k < 3; k++) {
            const bool open = !(limit > 0.f) || (p[1 + k] >= -limit && p[1 + k] <= limit);      // inclusive, as torch.clamp
            o[1 + k] = open ? p[0] * out[1 + k] : 0.f;
            o[4 + k] = tau * m[9 + k];
        }
        return;
    }
    if (vb > 1) {                                           // a lane per (set, coordinate)
        const int q = ((int)blockIdx.x - pose_blocks) * PS_FINISH_SETS + t;
        if (q >= 3 * B) return;
        const int b = q / 3, j = q % 3;
        float rot[PS_ROT];
        pose_stage(pose + (size_t)b * pose_stride, 0.f, limit, rot);
        float* gx = g_x + (size_t)b * V * 3 + j;
        for (int l = 0; l < L; l++) {
            const float* g = g_lm + ((size_t)b * L + l) * 3;
            const float gl[3] = {g[0], g[1], g[2]};
            float* d = gx + (size_t)landmarks[l] * 3;
            *d = *d + pose_pull(rot, rot[9], gl, j);
        }
        return;
    }
    // shared vertices: one workgroup
    for (int i = t; i < 3 * L; i += PS_FINISH_SETS) s_h[i] = 0.f;
    for (int b0 = 0; b0 < B; b0 += PS_STAGE) {
        const int n = min(PS_STAGE, B - b0);
        __syncthreads();
        if (t < n) pose_stage(pose + (size_t)(b0 + t) * pose_stride, 0.f, limit, s_rot[t]);
        __syncthreads();
        for (int i = t; i < 3 * L; i += PS_FINISH_SETS) {   // (element i is this lane's in every stage)
            const int l = i / 3, j = i % 3;
            float h = s_h[i];
            for (int k = 0; k < n; k++) {
                const float* g = g_lm + ((size_t)(b0 + k) * L + l) * 3;
                const float gl[3] = {g[0], g[1], g[2]};
                h += pose_pull(s_rot[k], s_rot[k][9], gl, j);
            }
            s_h[i] = h;
        }
    }
    __syncthreads();
    if (t < 3) {
        for (int l = 0; l < L; l++) {
            float* d = g_x + (size_t)landmarks[l] * 3 + t;
            *d = *d + s_h[3 * l + t];
        }
    }
}

}  // namespace d3m
