// d3m_camera_grad.h -- the gradient of the camera's PARAMETERS (d3m_camera_params_backward).
//
// The render nodes leave the gradient of the screen-space vertices, grad_screen [B,V,3] (what d3m_camera_backward takes to
// the mesh).  camera_point_grad_cam turns one (view, vertex) entry into the gradient gc of the camera-space point; then
//   look / look_at:  d rows += gc (x) (v - eye),   d eye -= R^T gc                         (12 sums: rows, sum gc)
//   projection:      d R += gc (x) v,  d t += gc,  d K[0..5] from (gu, gv') and (x'', y'', 1),  d dist from the
//                    distortion chain                                                        (23 sums)
// and the look / look_at rows go through the adjoint of the basis (z = normalise(at - eye) or normalise(direction),
// x = normalise(up x z), y = normalise(z x x); F.normalize(eps=1e-5): in the clamped branch the gradient does not flow
// through the norm).  Two stages in the FIXED order of d3m_set_sums.h, with WaveTree::XorButterfly, 12 or 23 sums (row
// stride 23, the tail stored as 0) and 1024 vertices per part up to 128 parts: k_camera_params_partial, then
// k_camera_params_finish, one workgroup that applies the basis adjoint to each view's sums and routes the rows.  The same
// bits on every run.
#pragma once
#include "d3m_aux.h"
#include "d3m_set_sums.h"

namespace d3m {

constexpr int CAM_SUMS = 23;            // the projection's sums (look / look_at use the first 12)
constexpr int CAM_ROW = 23;             // one view's gradients: projection R 9, t 3, K[0..5] 6, dist 5;
                                        // look / look_at eye 3, at_or_direction 3, up 3, rows 9
constexpr int CAM_OUT = 26;             // ... and the projection's K[6..8] (zeros, as the reference's)
constexpr int CAM_PER_PART = 1024;      // vertices per workgroup ...
constexpr int CAM_MAX_PARTS = 128;      // ... and workgroups per view

__host__ __device__ __forceinline__ int camera_parts(int V) { return set_parts(V, CAM_PER_PART, CAM_MAX_PARTS); }

// grid (parts, B): partial [B, parts, CAM_SUMS]
template <bool PROJ>
__global__ void __launch_bounds__(256) k_camera_params_partial(const float* __restrict__ vertices, int vb, Cam c,
                                                              const float* __restrict__ g_screen, int V,
                                                              float* __restrict__ partial) {
    constexpr int NS = PROJ ? 23 : 12;
    __shared__ float s_wave[4][NS];
    const int b = blockIdx.y, parts = gridDim.x;
    float acc[NS];
#pragma unroll
    for (int k = 0; k < NS; k++) acc[k] = 0.0f;
    const float* e = cam_ptr(c.eye_or_t, c.eye_b, b, 3);
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < V; i += (long)parts * 256) {
        const float* gp = g_screen + ((size_t)b * V + i) * 3;
        const float g[3] = {gp[0], gp[1], gp[2]};
        if (g[0] == 0 && g[1] == 0 && g[2] == 0) continue;
        const float* p = vertices + ((size_t)(vb > 1 ? b : 0) * V + i) * 3;
        const float v[3] = {p[0], p[1], p[2]};
        float gc[3];
        ProjTmp t;
        camera_point_grad_cam(c, b, v, g, gc, PROJ ? &t : nullptr);
        if (PROJ) {
#pragma unroll
            for (int r = 0; r < 3; r++) {
#pragma unroll
                for (int k = 0; k < 3; k++) acc[3 * r + k] += gc[r] * v[k];
                acc[9 + r] += gc[r];
            }
            const float* K = cam_ptr(c.K, c.K_b, b, 9);
            const float* dc = cam_ptr(c.dist, c.dist_b, b, 5);
            const float p1 = dc[2], p2 = dc[3];
            const float x_ = t.x_, y_ = t.y_, r2 = t.r2, r4 = r2 * r2, r6 = r4 * r2;
            const float x__ = x_ * t.radial + 2 * p1 * x_ * y_ + p2 * (r2 + 2 * x_ * x_);
            const float y__ = y_ * t.radial + p1 * (r2 + 2 * y_ * y_) + 2 * p2 * x_ * y_;
            const float gu = g[0] * 2.f / c.orig, gvp = -g[1] * 2.f / c.orig;
            acc[12] += gu * x__; acc[13] += gu * y__; acc[14] += gu;
            acc[15] += gvp * x__; acc[16] += gvp * y__; acc[17] += gvp;
            const float gx2 = K[0] * gu + K[3] * gvp, gy2 = K[1] * gu + K[4] * gvp;
            const float gr = gx2 * x_ + gy2 * y_;          // d / d radial
            acc[18] += gr * r2;
            acc[19] += gr * r4;
            acc[20] += gx2 * (2 * x_ * y_) + gy2 * (r2 + 2 * y_ * y_);
            acc[21] += gx2 * (r2 + 2 * x_ * x_) + gy2 * (2 * x_ * y_);
            acc[22] += gr * r6;
        } else {
            const float d[3] = {v[0] - e[0], v[1] - e[1], v[2] - e[2]};
#pragma unroll
            for (int r = 0; r < 3; r++) {
#pragma unroll
                for (int k = 0; k < 3; k++) acc[3 * r + k] += gc[r] * d[k];
                acc[9 + r] += gc[r];
            }
        }
    }
    set_store_partial<NS, WaveTree::XorButterfly, CAM_SUMS>(acc, s_wave, partial, b, parts);
}

// adjoint of u = v / max(|v|, 1e-5) (normalize3): gu -> gv
__device__ __forceinline__ void normalize3_adjoint(const float* v, const float* gu, float* gv) {
    const float n = sqrtf(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
    const float d = fmaxf(n, 1e-5f);
    const float vg = v[0] * gu[0] + v[1] * gu[1] + v[2] * gu[2];
    const float s = n >= 1e-5f ? vg / (d * d * n) : 0.0f;      // (clamped: the norm is a constant)
#pragma unroll
    for (int k = 0; k < 3; k++) gv[k] = gu[k] / d - v[k] * s;
}

// The basis' vectors (d3m_basis) as the finish kernel reads them; `on` == 0: none (the rows are constants)
struct CamBasis {
    const float *eye, *at, *up;
    int eye_b, at_b, up_b, is_look_at, on;
};

struct CamGradOut {
    float *eye_or_t, *at, *up, *rot, *K, *dist;
    int eye_b, at_b, up_b, rot_b, K_b, dist_b;
};

// One workgroup.  rows [B, CAM_ROW]: each view's gradients (workspace); `out` the parameters' gradients (NULL skipped).
__global__ void __launch_bounds__(256) k_camera_params_finish(Cam c, CamBasis bs, const float* __restrict__ partial, int B,
                                                             int parts, float* __restrict__ rows, CamGradOut out) {
    const bool proj = c.mode == D3M_CAMERA_PROJECTION;
    for (int b = threadIdx.x; b < B; b += 256) {
        float s[CAM_SUMS];
        set_add_parts(partial, b, parts, s);
        float* row = rows + (size_t)b * CAM_ROW;
        if (proj) {
#pragma unroll
            for (int k = 0; k < CAM_ROW; k++) row[k] = s[k];
            continue;
        }
        const float* r = cam_ptr(c.rot, c.rot_b, b, 9);
        float ge[3] = {0, 0, 0}, ga[3] = {0, 0, 0}, gup[3] = {0, 0, 0};
        if (bs.on) {
            // the basis again (k_camera_basis), keeping the vectors before each normalisation
            const float* e = cam_ptr(bs.eye, bs.eye_b, b, 3);
            const float* a = cam_ptr(bs.at, bs.at_b, b, 3);
            const float* u = cam_ptr(bs.up, bs.up_b, b, 3);
            float z0[3], z[3], x0[3], x[3], y0[3];
            for (int k = 0; k < 3; k++) z0[k] = z[k] = bs.is_look_at ? a[k] - e[k] : a[k];
            normalize3(z);
            cross3(u, z, x0);
            for (int k = 0; k < 3; k++) x[k] = x0[k];
            normalize3(x);
            cross3(z, x, y0);
            float gx[3] = {s[0], s[1], s[2]}, gz[3] = {s[6], s[7], s[8]};
            const float gy[3] = {s[3], s[4], s[5]};
            float gy0[3], gx0[3], gz0[3], t[3];
            normalize3_adjoint(y0, gy, gy0);            // y = normalise(z x x)
            cross3(x, gy0, t);
            for (int k = 0; k < 3; k++) gz[k] += t[k];
            cross3(gy0, z, t);
            for (int k = 0; k < 3; k++) gx[k] += t[k];
            normalize3_adjoint(x0, gx, gx0);            // x = normalise(up x z)
            cross3(z, gx0, gup);
            cross3(gx0, u, t);
            for (int k = 0; k < 3; k++) gz[k] += t[k];
            normalize3_adjoint(z0, gz, gz0);            // z = normalise(at - eye) or normalise(direction)
            for (int k = 0; k < 3; k++) {
                ga[k] = gz0[k];
                ge[k] = bs.is_look_at ? -gz0[k] : 0.0f;
            }
        }
        // ... then the translation: d eye -= R^T sum gc
#pragma unroll
        for (int k = 0; k < 3; k++) {
            row[k] = ge[k] - ((r[k] * s[9] + r[3 + k] * s[10]) + r[6 + k] * s[11]);
            row[3 + k] = ga[k];
            row[6 + k] = gup[k];
        }
#pragma unroll
        for (int k = 0; k < 9; k++) row[9 + k] = s[k];
    }
    __syncthreads();
    set_route_rows<CAM_ROW, CAM_OUT>(rows, B, [&](int j) -> SetRoute {
        if (proj) {
            if (j < 9) return {out.rot, out.rot_b, j, 9, false};
            if (j < 12) return {out.eye_or_t, out.eye_b, j - 9, 3, false};
            if (j < 18) return {out.K, out.K_b, j - 12, 9, false};
            if (j < 23) return {out.dist, out.dist_b, j - 18, 5, false};
            return {out.K, out.K_b, j - 17, 9, true};                          // K's last row: zeros
        }
        if (j < 3) return {out.eye_or_t, out.eye_b, j, 3, false};
        if (j < 6) return {out.at, out.at_b, j - 3, 3, false};
        if (j < 9) return {out.up, out.up_b, j - 6, 3, false};
        if (j < 18) return {out.rot, out.rot_b, j - 9, 9, false};
        return {nullptr, 1, 0, 3, false};
    });
}

}  // namespace d3m
