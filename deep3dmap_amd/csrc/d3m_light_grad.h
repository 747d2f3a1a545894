// d3m_light_grad.h -- the gradient of the light's PARAMETERS (d3m_light_params_backward).
//
// The lit render node leaves the gradient of its per-face light, grad_light [Bl,F',3] (d3m_backward_textures_lit).  With
// light[b,f] = ia*ca + id*cd*r, r = relu(n.d) (face_light), summed over the faces of light row b and G = grad_light[b,f]:
//   d ia = ca . sum G            d ca = ia * sum G
//   d id = cd . sum r G          d cd = id * sum r G          d dir = id * sum [n.d > 0] (G . cd) n
// so one pass over the faces reduces nine sums per row; a term whose intensity is 0 is skipped (lighting.py:36,40) and its
// parameters get zeros.  Two stages in the FIXED order of d3m_set_sums.h, with WaveTree::XorButterfly, 9 sums and 1024 faces
// per part up to 128 parts: k_light_params_partial, then k_light_params_finish, one workgroup that forms each row's
// gradients from its sums and routes them.  The same bits on every run, in every mode.
#pragma once
#include "d3m_aux.h"
#include "d3m_set_sums.h"

namespace d3m {

constexpr int LIGHT_SUMS = 9;           // sum G, sum r G, sum [n.d > 0] (G . cd) n
constexpr int LIGHT_PARAMS = 11;        // ia, id, ca[3], cd[3], dir[3]
constexpr int LIGHT_PER_PART = 1024;    // faces per workgroup ...
constexpr int LIGHT_MAX_PARTS = 128;    // ... and workgroups per light row

__host__ __device__ __forceinline__ int light_parts(int Fp) { return set_parts(Fp, LIGHT_PER_PART, LIGHT_MAX_PARTS); }

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
    set_store_partial<LIGHT_SUMS, WaveTree::XorButterfly>(acc, s_wave, partial, b, parts);
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
        set_add_parts(partial, b, parts, s);
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
    set_route_rows<LIGHT_PARAMS, LIGHT_PARAMS>(rows, Bl, [&](int j) -> SetRoute {
        if (j == 0) return {out.ia, out.ia_b, 0, 1, false};
        if (j == 1) return {out.id, out.id_b, 0, 1, false};
        if (j < 5) return {out.ca, out.ca_b, j - 2, 3, false};
        if (j < 8) return {out.cd, out.cd_b, j - 5, 3, false};
        return {out.dir, out.dir_b, j - 8, 3, false};
    });
}

}  // namespace d3m
