// d3m_light_grad.h -- the gradient of the light's PARAMETERS (d3m_light_params_backward).
//
// The lit render node leaves the gradient of its per-face light, grad_light [Bl,F',3] (d3m_backward_textures_lit).  With
// light[b,f] = ia*ca + id*cd*r, r = relu(n.d) (face_light), summed over the faces of light row b and G = grad_light[b,f]:
//   d ia = ca . sum G            d ca = ia * sum G
//   d id = cd . sum r G          d cd = id * sum r G          d dir = id * sum [n.d > 0] (G . cd) n
// so one pass over the faces reduces nine sums per row; a term whose intensity is 0 is skipped (lighting.py:36,40) and its
// parameters get zeros.  Two stages in a FIXED order, no float atomics: k_light_params_partial -- per-workgroup partials,
// each lane's faces in ascending order, butterfly sums within the wave, the waves in order -- then k_light_params_finish, one
// workgroup that adds the partials in order, forms each row's gradients and sums the rows of a parameter of batch 1 in view
// order.  The same bits on every run, in every mode.
#pragma once
#include "d3m_aux.h"

namespace d3m {

constexpr int LIGHT_SUMS = 9;           // sum G, sum r G, sum [n.d > 0] (G . cd) n
constexpr int LIGHT_PARAMS = 11;        // ia, id, ca[3], cd[3], dir[3]
constexpr int LIGHT_MAX_PARTS = 128;    // workgroups per light row

__host__ __device__ __forceinline__ int light_parts(int Fp) {
    const int n = (Fp + 1023) / 1024;
    return n < 1 ? 1 : (n > LIGHT_MAX_PARTS ? LIGHT_MAX_PARTS : n);
}

// grid (parts, Bl): partial [Bl, parts, 9]
__global__ void __launch_bounds__(256) k_light_params_partial(IndexedFaces fs, DevLight dl, const float* __restrict__ g_light,
                                                             float* __restrict__ partial) {
    __shared__ float s_wave[4][LIGHT_SUMS];
    const int b = blockIdx.y, parts = gridDim.x;
    const int Fp = fs.num_faces();
    const LightParams lp = light_at(dl, b);
    float acc[LIGHT_SUMS];
#pragma unroll
    for (int k = 0; k < LIGHT_SUMS; k++) acc[k] = 0.0f;
    for (long f = (long)blockIdx.x * 256 + threadIdx.x; f < Fp; f += (long)parts * 256) {
        const size_t i = (size_t)b * Fp + f;
        const float g[3] = {g_light[3 * i], g_light[3 * i + 1], g_light[3 * i + 2]};
        if (g[0] == 0 && g[1] == 0 && g[2] == 0) continue;
        float fc[9], l[3], nrm[3], len, cs;
        fs.load(b, (int)f, fc);
        face_light(fc, lp, l, nrm, &len, &cs);
        const float r = fmaxf(cs, 0.0f);
        const float gd = cs > 0 ? g[0] * lp.cd[0] + g[1] * lp.cd[1] + g[2] * lp.cd[2] : 0.0f;
#pragma unroll
        for (int k = 0; k < 3; k++) {
            acc[k] += g[k];
            acc[3 + k] += r * g[k];
            acc[6 + k] += gd * nrm[k];
        }
    }
#pragma unroll
    for (int k = 0; k < LIGHT_SUMS; k++) {
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) acc[k] += __shfl_xor(acc[k], off, 64);
    }
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < LIGHT_SUMS; k++) s_wave[wave][k] = acc[k];
    }
    __syncthreads();
    if (threadIdx.x < LIGHT_SUMS) {
        const int k = threadIdx.x;
        partial[((size_t)b * parts + blockIdx.x) * LIGHT_SUMS + k] = ((s_wave[0][k] + s_wave[1][k]) + s_wave[2][k]) + s_wave[3][k];
    }
}

// One workgroup.  rows [Bl, 11]: each row's gradients (workspace); `out` the parameters' gradients (NULL fields skipped).
struct LightGradOut {
    float *ia, *id, *ca, *cd, *dir;
    int ia_b, id_b, ca_b, cd_b, dir_b;
};
__global__ void __launch_bounds__(256) k_light_params_finish(DevLight dl, const float* __restrict__ partial, int Bl, int parts,
                                                            float* __restrict__ rows, LightGradOut out) {
    for (int b = threadIdx.x; b < Bl; b += 256) {
        float s[LIGHT_SUMS];
#pragma unroll
        for (int k = 0; k < LIGHT_SUMS; k++) s[k] = 0.0f;
        for (int p = 0; p < parts; p++) {
#pragma unroll
            for (int k = 0; k < LIGHT_SUMS; k++) s[k] += partial[((size_t)b * parts + p) * LIGHT_SUMS + k];
        }
        const LightParams lp = light_at(dl, b);
        const bool amb = lp.ia != 0, dir = lp.id != 0;
        float* row = rows + (size_t)b * LIGHT_PARAMS;
        row[0] = amb ? (lp.ca[0] * s[0] + lp.ca[1] * s[1]) + lp.ca[2] * s[2] : 0.0f;
        row[1] = dir ? (lp.cd[0] * s[3] + lp.cd[1] * s[4]) + lp.cd[2] * s[5] : 0.0f;
#pragma unroll
        for (int k = 0; k < 3; k++) {
            row[2 + k] = amb ? lp.ia * s[k] : 0.0f;
            row[5 + k] = dir ? lp.id * s[3 + k] : 0.0f;
            row[8 + k] = dir ? lp.id * s[6 + k] : 0.0f;
        }
    }
    __syncthreads();
    // parameter j of the row -> (output, its batch, column)
    for (int e = threadIdx.x; e < LIGHT_PARAMS * (Bl + 1); e += 256) {
        const int b = e / LIGHT_PARAMS, j = e % LIGHT_PARAMS;      // b == Bl: the sum over the rows (parameters of batch 1)
        float* dst;
        int nb, col, width;
        if (j == 0) { dst = out.ia; nb = out.ia_b; col = 0; width = 1; }
        else if (j == 1) { dst = out.id; nb = out.id_b; col = 0; width = 1; }
        else if (j < 5) { dst = out.ca; nb = out.ca_b; col = j - 2; width = 3; }
        else if (j < 8) { dst = out.cd; nb = out.cd_b; col = j - 5; width = 3; }
        else { dst = out.dir; nb = out.dir_b; col = j - 8; width = 3; }
        if (!dst) continue;
        if (nb > 1 && b < Bl) {
            dst[(size_t)b * width + col] = rows[(size_t)b * LIGHT_PARAMS + j];
        } else if (nb <= 1 && b == Bl) {
            float t = 0.0f;
            for (int r = 0; r < Bl; r++) t += rows[(size_t)r * LIGHT_PARAMS + j];
            dst[col] = t;
        }
    }
}

}  // namespace d3m
