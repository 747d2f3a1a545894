// d3m_fragment_geometry.h -- the INTERIOR geometry gradient of everything drawn over a coverage record (AttrMaps,
// d3m_fragments.h): the derivative of the perspective-correct weights u_c of each owned pixel with respect to the owner's
// three screen-space corners, as ONE adjoint that the attribute images (d3m_attributes.h), the plain bilinear uv texture
// images (d3m_uv_texture.h) and the weight map itself (k_fragment_weights) share.  Coverage -- which face owns which pixel --
// is a constant: the silhouette gradient is the business of the render nodes' edge pass, not of this header.
//
// The function that is differentiated.  Internal pixel p = (xi, yi) of view b with owner fn >= 0, corners (x_c, y_c, z_c) =
// faces[b,fn,c,:] (= screen_vertices[b, tri[fn][c]], or tri[fn - F][2 - c] for a fill_back copy), centre xp = (2 xi + 1 - S) /
// S, yp likewise:
//   b   = M^-1 (xp, yp, 1)^T,  M = [[x0,x1,x2],[y0,y1,y2],[1,1,1]]   (raw barycentrics)
//   u_c = (b_c / z_c) / sum_k (b_k / z_k)
// -- what weight_map * depth_map / z_c evaluates with the rasteriser's clamp-and-renormalise of b taken as the identity (at an
// owned pixel it only absorbs rounding; differentiating through it would make the gradient jump at pixels whose centre lies
// on an edge).  The adjoint evaluates b, d = 1 / sum_k (b_k / z_k) and u from the CORNERS, not from the maps: b_c = N[c][0]
// (xp - x2) + N[c][1] (yp - y2) for c = 0, 1 and b_2 = (1 - b_0) - b_1 -- differences of coordinates only, where the
// rasteriser's pixel-space inverse loses digits on thin faces (the maps' u is up to 1e-5 away on a sliver) -- and so reads
// nothing but the owner index and h of a pixel.  With h_c = dL/du_c (the per-pixel input of the adjoint, h [B,S,S,3] in the
// maps' orientation), hbar = (u_0 h_0 + u_1 h_1) + u_2 h_2 and e_c = h_c - hbar:
//   A_c    = dL/db_c = (d / z_c) e_c
//   dL/dz_k          = -(u_k / z_k) e_k
//   dL/dx_k          = -b_k Px,  Px = (N[0][0] A_0 + N[1][0] A_1) + N[2][0] A_2
//   dL/dy_k          = -b_k Py,  Py = (N[0][1] A_0 + N[1][1] A_1) + N[2][1] A_2
// N = the first two columns of M^-1, formed per face in NDC from corner DIFFERENCES (no S / 2 factor, no cancellation of
// products of coordinates): den = (x1 - x0)(y2 - y0) - (x2 - x0)(y1 - y0), N[c][0] = (y_{c+1} - y_{c+2}) / den, N[c][1] =
// (x_{c+2} - x_{c+1}) / den (indices mod 3).
//
// The per-pixel h of the two image nodes, sg[k] = scale * g[b,k,out(p)] (va_pixel_grads), written by one lane per internal
// pixel, channels walked in chunks of 8, every element of h written (an uncovered pixel: +0):
//   attributes   h_c = sum over k = 0, 1, ... (from 0, ascending) of sg[k] * a_c[k];
//   uv texture   (plain bilinear only) Dx = sum over k ascending of sg[k] * ((1 - fy)(t01 - t00) + fy (t11 - t10)), Dy = sum
//                of sg[k] * ((1 - fx)(t10 - t00) + fx (t11 - t01)), t00, t10, t01, t11 the taps bilinear_taps chose (p00 =
//                (yi, xi), p10 = (y1, xi), p01 = (yi, x1), p11 = (y1, x1)) at the FORWARD's pos (uvt_pixel_position, from the
//                maps: the slope of the very patch the forward evaluated), fx = pos_x - xi, fy = pos_y - yi; Dx (Dy) = 0 where
//                pos_x (pos_y) sits at a clamp limit (<= 0 or >= size - 1); h_c = (W - 1) cx_c Dx + (H - 1) cy_c Dy with the
//                wrapped corner uv of uvt_pixel_position (a fill_back copy: corners 2 - c).  faces_uv is a constant.
//                FgUvSlopes below is the one statement of Dx, Dy and this h_c; the SH-shaded uv albedo
//                (d3m_sh_uv_fragments.h) calls it with dL/da_k in the place of sg[k] and adds its normals' term.
// Going through h costs 12 B a pixel each way -- small beside reading g for C channels -- and keeps one shared adjoint.
//
// THE ORDER of the adjoint's sums, the same bits on every run (no float atomics anywhere, nothing is cleared):
//   1. per visible face (b, fn), corner k, coordinate j in {x, y, z}:  Gv[b,fn,k,j] = the sum over the pixels the face owns of
//      the pixel's term above (fg_add_pixel).  Route and order: stage 1 of d3m_fragments.h (THE ORDER there), with 9
//      accumulators a face.  Gv [B,F',3,3] is stored plainly; entries of faces that own no pixel are never written or read.
//   2. per vertex v, view b, coordinate j: stage 2 of the attribute adjoint with C = 3 and a per-view result
//      (k_vertex_attribute_adjoint_chunks / k_vertex_attribute_adjoint_rows, the SAME kernels: Gv has G's layout [B,F',3,C]):
//      acc = 0; for the items 3 f + c of the vertex's adjacency row in ascending order: acc += Gv[b,f,c,j] if face f is
//      visible in view b, then -- fill_back -- acc += Gv[b,F+f,2-c,j] if the copy is; long rows through the chunks of
//      d3m_row_gather.h.  A vertex of no visible face gets an exact +0.
// Launches: k_fragment_weights 1; the shared adjoint 3 (two face-sum kernels, the rows) and the chunks on a mesh with long
// rows; a node adds 1 for its h.
#pragma once
#include "d3m_attributes.h"
#include "d3m_uv_texture.h"

namespace d3m {

// ---- the weight map: one lane per internal pixel; every element of u [B,S,S,3] is written (an uncovered pixel: +0) ----------
__global__ void __launch_bounds__(256) k_fragment_weights(AttrMaps m, float* __restrict__ u_map) {
    const long p = (long)blockIdx.x * 256 + threadIdx.x;
    int b, x, y, fn;
    if (!fr_pixel(m, p, b, x, y, fn)) return;
    float u[3] = {0.0f, 0.0f, 0.0f};
    if (fn >= 0) {
        float z[3];
        fr_corner_depths(m, b, fn, z);
        va_weights(m, (size_t)p, z, u);
    }
#pragma unroll
    for (int c = 0; c < 3; c++) u_map[3 * (size_t)p + c] = u[c];
}

// ---- the shared adjoint, stage 1 ------------------------------------------------------------------------------------------
// what a face contributes to every one of its pixels' terms
struct FgFace {
    float z[3];
    float nx[3], ny[3];                  // N[c][0], N[c][1]
    float x2, y2;                        // corner 2: b_c = N[c][0] (xp - x2) + N[c][1] (yp - y2) for c = 0, 1
};

// den != 0 for a face that owns a pixel (the rasteriser gives a zero-area face none).  A degenerate face that is merely
// LISTED gets Inf or NaN here, which only fg_add_pixel would multiply -- and that is not reached without an owned pixel.
__device__ __forceinline__ void fg_face(const float* face, FgFace& f) {
    const float x0 = face[0], y0 = face[1], x1 = face[3], y1 = face[4], x2 = face[6], y2 = face[7];
    const float den = (x1 - x0) * (y2 - y0) - (x2 - x0) * (y1 - y0);
    f.z[0] = face[2]; f.z[1] = face[5]; f.z[2] = face[8];
    f.nx[0] = (y1 - y2) / den; f.nx[1] = (y2 - y0) / den; f.nx[2] = (y0 - y1) / den;
    f.ny[0] = (x2 - x1) / den; f.ny[1] = (x0 - x2) / den; f.ny[2] = (x1 - x0) / den;
    f.x2 = x2; f.y2 = y2;
}

// adds the nine terms (corner-major: acc[3 k + j]) of internal pixel (x, y), index q into the batch's maps, onto acc
__device__ __forceinline__ void fg_add_pixel(const FgFace& f, const float* __restrict__ h, size_t q, int x, int y, int S,
                                             float* acc) {
    const float dx = pixel_center(x, S) - f.x2, dy = pixel_center(y, S) - f.y2;
    float b[3], t[3], u[3], e[3], A[3];
    b[0] = f.nx[0] * dx + f.ny[0] * dy;
    b[1] = f.nx[1] * dx + f.ny[1] * dy;
    b[2] = (1.0f - b[0]) - b[1];
#pragma unroll
    for (int c = 0; c < 3; c++) t[c] = b[c] / f.z[c];
    const float d = 1.0f / ((t[0] + t[1]) + t[2]);
#pragma unroll
    for (int c = 0; c < 3; c++) u[c] = t[c] * d;
    const float h0 = h[3 * q], h1 = h[3 * q + 1], h2 = h[3 * q + 2];
    const float hbar = (u[0] * h0 + u[1] * h1) + u[2] * h2;
    e[0] = h0 - hbar; e[1] = h1 - hbar; e[2] = h2 - hbar;
#pragma unroll
    for (int c = 0; c < 3; c++) A[c] = (d / f.z[c]) * e[c];
    const float px = (f.nx[0] * A[0] + f.nx[1] * A[1]) + f.nx[2] * A[2];
    const float py = (f.ny[0] * A[0] + f.ny[1] * A[1]) + f.ny[2] * A[2];
#pragma unroll
    for (int k = 0; k < 3; k++) {
        acc[3 * k + 0] += -b[k] * px;
        acc[3 * k + 1] += -b[k] * py;
        acc[3 * k + 2] += -(u[k] / f.z[k]) * e[k];
    }
}

// fr_face_sums / fr_large_face_sums (d3m_fragments.h) with nine accumulators
struct FgFaceSums {
    const AttrMaps& m;
    const float* h;
    float* Gv;
    FgFace f;
    __device__ __forceinline__ void setup(const float* face, int) { fg_face(face, f); }
    __device__ __forceinline__ void add(int x, int y, size_t q, float* acc) const { fg_add_pixel(f, h, q, x, y, m.S, acc); }
    __device__ __forceinline__ void store(size_t gi, const float* acc) const {
#pragma unroll
        for (int k = 0; k < 9; k++) Gv[gi * 9 + k] = acc[k];
    }
};

__global__ void __launch_bounds__(256) k_fragment_geometry_face_sums(AttrMaps m, const float* __restrict__ h,
                                                                    const int* __restrict__ list,
                                                                    const int* __restrict__ n_list, float* __restrict__ Gv) {
    FgFaceSums policy{m, h, Gv};
    fr_face_sums<9>(m, list, n_list, policy);
}

__global__ void __launch_bounds__(RG_BLOCK) k_fragment_geometry_large_face_sums(AttrMaps m, const float* __restrict__ h,
                                                                               const int* __restrict__ list,
                                                                               const int* __restrict__ n_list,
                                                                               float* __restrict__ Gv) {
    FgFaceSums policy{m, h, Gv};
    fr_large_face_sums<9>(m, list, n_list, policy);
}

// ---- the nodes' h: one lane per internal pixel (fr_pixel) --------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_vertex_attribute_pixel_grads(AttrMaps m, const float* __restrict__ attributes,
                                                                     int attr_batch, int V, int C,
                                                                     const float* __restrict__ grad_images,
                                                                     float* __restrict__ h) {
    const long p = (long)blockIdx.x * 256 + threadIdx.x;
    int b, x, y, fn;
    if (!fr_pixel(m, p, b, x, y, fn)) return;
    float acc[3] = {0.0f, 0.0f, 0.0f};
    if (fn >= 0) {
        const int s = fr_output_size(m);
        const bool back = fn >= m.Ft;
        const int32_t* t = m.tri + (size_t)(back ? fn - m.Ft : fn) * 3;
        const float* attr = attributes + (size_t)(attr_batch > 1 ? b : 0) * V * C;
        const float* a[3] = {attr + (size_t)(back ? t[2] : t[0]) * C, attr + (size_t)t[1] * C,
                             attr + (size_t)(back ? t[0] : t[2]) * C};
        const float* g_view = grad_images + (size_t)b * C * s * s;
        for (int k0 = 0; k0 < C; k0 += VA_CHUNK) {
            float gs[VA_CHUNK];
            va_pixel_grads(m, g_view, C, k0, x, y, gs);
#pragma unroll
            for (int kk = 0; kk < VA_CHUNK; kk++) {
                if (k0 + kk >= C) continue;
#pragma unroll
                for (int c = 0; c < 3; c++) acc[c] += gs[kk] * a[c][k0 + kk];
            }
        }
    }
#pragma unroll
    for (int c = 0; c < 3; c++) h[3 * (size_t)p + c] = acc[c];
}

// The bilinear lookup's slopes along pos, stated once for the two nodes that differentiate it (this header's uv texture node
// and d3m_sh_uv_fragments.h).  fg_uv_slopes: the four taps bilinear_taps chose at (pos_x, pos_y) of one image [H,W,C] and the
// fractions.  add(c, g, dx, dy): dx += g * (channel c's slope along pos_x), dy likewise.  finish(k, dx, dy, h): the derivative
// of the clamp is 0 AT a limit; h_c = (W - 1) cx_c dx + (H - 1) cy_c dy.
struct FgUvSlopes {
    const float *t00, *t10, *t01, *t11;
    float fx, fy, x_max, y_max;
    bool inside_x, inside_y;
    __device__ __forceinline__ void add(int c, float g, float& dx, float& dy) const {
        const float a00 = t00[c], a10 = t10[c], a01 = t01[c], a11 = t11[c];
        dx += g * ((1.0f - fy) * (a01 - a00) + fy * (a11 - a10));
        dy += g * ((1.0f - fx) * (a10 - a00) + fx * (a11 - a01));
    }
    __device__ __forceinline__ void finish(const UvtCorners& k, float dx, float dy, float* h) const {
        if (!inside_x) dx = 0.0f;
        if (!inside_y) dy = 0.0f;
#pragma unroll
        for (int c = 0; c < 3; c++) h[c] = x_max * k.cx[c] * dx + y_max * k.cy[c] * dy;
    }
};

__device__ __forceinline__ FgUvSlopes fg_uv_slopes(const UvTexture& tx, const float* __restrict__ img, float pos_x, float pos_y) {
    TexelTaps tt;
    bilinear_taps(pos_x, pos_y, tx.H, tx.W, tt);
    FgUvSlopes s;
    s.t00 = img + (size_t)tt.pix[0] * tx.C;
    s.t10 = img + (size_t)tt.pix[1] * tx.C;
    s.t01 = img + (size_t)tt.pix[2] * tx.C;
    s.t11 = img + (size_t)tt.pix[3] * tx.C;
    s.fx = pos_x - (float)(int)pos_x;
    s.fy = pos_y - (float)(int)pos_y;
    s.x_max = (float)(tx.W - 1);
    s.y_max = (float)(tx.H - 1);
    s.inside_x = pos_x > 0.0f && pos_x < s.x_max;
    s.inside_y = pos_y > 0.0f && pos_y < s.y_max;
    return s;
}

__global__ void __launch_bounds__(256) k_uv_texture_pixel_grads(AttrMaps m, UvTexture tx, const float* __restrict__ image,
                                                               const float* __restrict__ grad_images, float* __restrict__ h) {
    const long p = (long)blockIdx.x * 256 + threadIdx.x;
    int b, x, y, fn;
    if (!fr_pixel(m, p, b, x, y, fn)) return;
    float out[3] = {0.0f, 0.0f, 0.0f};
    if (fn >= 0) {
        const int s = fr_output_size(m), C = tx.C;
        float z[3];
        fr_corner_depths(m, b, fn, z);
        UvtCorners k;
        float pos_x, pos_y;
        uvt_pixel_position(m, tx, (size_t)p, fn, z, k, pos_x, pos_y);
        const FgUvSlopes sl = fg_uv_slopes(tx, image + (size_t)(tx.image_batch > 1 ? b : 0) * tx.H * tx.W * C, pos_x, pos_y);
        const float* g_view = grad_images + (size_t)b * C * s * s;
        float dx = 0.0f, dy = 0.0f;
        for (int k0 = 0; k0 < C; k0 += UVT_CHUNK) {
            float gs[VA_CHUNK];
            static_assert(UVT_CHUNK == VA_CHUNK, "va_pixel_grads walks the nodes' one chunk size");
            va_pixel_grads(m, g_view, C, k0, x, y, gs);
#pragma unroll
            for (int kk = 0; kk < VA_CHUNK; kk++) {
                const int c = k0 + kk;
                if (c >= C) continue;
                sl.add(c, gs[kk], dx, dy);
            }
        }
        sl.finish(k, dx, dy, out);
    }
#pragma unroll
    for (int c = 0; c < 3; c++) h[3 * (size_t)p + c] = out[c];
}

}  // namespace d3m
