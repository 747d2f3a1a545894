// d3m_sh_fragments.h -- per-pixel spherical-harmonic shading over a coverage record (AttrMaps, d3m_fragments.h): per-vertex
// normals and, optionally, per-vertex albedo interpolated at every pixel, the normal normalised PER PIXEL, the 9-term light of
// d3m_smooth_shade.h evaluated there, and the adjoint with respect to the normals, the albedo, the light and -- through the
// shared adjoint of d3m_fragment_geometry.h -- the screen vertices (neural_renderer/sh_fragments.py).
//
// THE FUNCTION.  Internal pixel p of view b with owner fn >= 0: f = fn mod F, corner c of the owner is vertex v_c = tri[f][c]
// (fn < F) or tri[f][2 - c] (the fill_back copy: d3m_attributes.h), u_c = weight_map[b,p,c] * (depth_map[b,p] / z_c)
// (va_weights), n_c = normals[v_c], c_c = colors[v_c]:
//   m   = (u_0 n_0 + u_1 n_1) + u_2 n_2        r = sqrt((m_x^2 + m_y^2) + m_z^2)        n = m / max(r, 1e-6)
//   s_k = sum over j = 0..8, ascending, from the first product, of sh[b,k,j] H_j(n)     (ss_basis / ss_light; no clamp, no ReLU)
//   a   = (u_0 c_0 + u_1 c_1) + u_2 c_2        value_k = a_k s_k                        (no colours: value_k = s_k)
// The normal is NOT flipped for a pixel a back copy owns.  An uncovered pixel takes background[k] (NULL: 0).  The image is what
// fr_output_pixel_walk makes of that map: rows reversed and, with anti-aliasing, ((p00 + p01) + p10) + p11 in OUTPUT
// orientation, times 1/4, background included.  alpha: the bits of k_vertex_attribute_images' alpha.
//
// THE ADJOINT, for g = dL/dimages and sg_k = scale g[b,k,out(p)] (scale = 1 or 1/4: va_pixel_grads).  Per covered internal
// pixel, everything recomputed from the record and the inputs (nothing is kept from the forward):
//   ga_k = sg_k s_k   (dL/da_k)          gs_k = sg_k a_k   (dL/ds_k; no colours: sg_k)
//   gn   = sum over k = 0, 1, 2, from 0, of gs_k * (d s_k / d n)                         (ss_light_gradient)
//   gm   = (gn - n ((n_x gn_x + n_y gn_y) + n_z gn_z)) / r  where r >= 1e-6,  gn / 1e-6  elsewhere   (dL/dm, of the expression as written)
//   h_c  = ((gm_x n_c.x + gm_y n_c.y) + gm_z n_c.z) + ((ga_0 c_c.0 + ga_1 c_c.1) + ga_2 c_c.2)       (dL/du_c; no colours: the first)
// THE ORDER of every sum, the same bits on every run (no float atomics anywhere, nothing is cleared):
//   sh       27 sums per view (k-major: 9 k + j) of gs_k H_j(n) over the view's covered internal pixels, through the tree of
//            d3m_set_sums.h: a set is a view, an element an internal pixel (index y S + x of the maps; an uncovered one adds
//            nothing), N = SHF_SUMS = 27, PER_PART = SHF_PER_PART = 1024, MAX_PARTS = SHF_MAX_PARTS = 256,
//            WaveTree::DppRows.  k_sh_fragment_finish is its step 4; a shared sh [3,9] takes each view's sum first, then the
//            views in ascending order, starting from view 0's value.
//   normals, colours   the per-pixel kernel leaves gm and ga as a GRADIENT IMAGE Q at the internal size, in output orientation
//            (rows reversed), channel planes [*, S, S]; the attribute adjoint (d3m_attributes.h, THE ORDER there: per visible
//            face the sums over the pixels it owns, a workgroup for a face whose box exceeds FM_MAX_BBOX_AREA pixels; then per
//            vertex over the adjacency, long rows through the chunks of d3m_row_gather.h; shared inputs over the views in
//            ascending order) reads Q as the image gradient of a record re-labelled image_size = S, anti_aliasing = 0 over
//            the same maps (the scale is already in Q) -- the SAME kernels, no copy of them.  Only what is wanted is written
//            and gathered: normals AND colours of one batch size are ONE gather of C = 6 channels, Q [B,6,S,S] -> [batch,V,6];
//            otherwise a gather of C = 3 per wanted gradient, each over its own Q block [B,3,S,S] (gm's first).  Q is written
//            at covered pixels only and read at owned pixels only.
//   screen vertices    h [B,S,S,3] (every element written, +0 where uncovered; the same per-pixel launch writes it) goes to
//            d3m_fragment_geometry_backward.
//
// Launches.  Forward: k_sh_fragment_images.  Backward: k_sh_fragment_backward_pixels, k_sh_fragment_finish (grad_sh only),
// and per gather k_vertex_attribute_face_sums, k_vertex_attribute_large_face_sums, k_vertex_attribute_adjoint_rows, with
// k_vertex_attribute_adjoint_chunks on a mesh with long rows.
#pragma once
#include "d3m_attributes.h"
#include "d3m_set_sums.h"
#include "d3m_smooth_shade.h"

namespace d3m {

constexpr int SHF_SUMS = SS_SUMS;       // N: grad_sh of one view, 3 channels x 9 terms
constexpr int SHF_PER_PART = 1024;      // PER_PART: internal pixels per part (four per lane)
constexpr int SHF_MAX_PARTS = 256;      // MAX_PARTS: reached at S = 512; beyond it the lanes stride further
constexpr WaveTree SHF_TREE = WaveTree::DppRows;

__host__ __device__ __forceinline__ int shf_parts(long pixels) { return set_parts(pixels, SHF_PER_PART, SHF_MAX_PARTS); }

// The per-vertex inputs as the kernels read them: normals [nb,V,3], colors [cb,V,3] or NULL, sh [sb,3,9]
struct ShfInputs {
    const float* normals;
    const float* colors;
    const float* sh;
    int nb, cb, sb, V;
};

// what a covered internal pixel evaluates
struct ShfPixel {
    float u[3];
    int ids[3];
    float n[3], r;
    float H[9];
    float a[3];                          // the interpolated albedo (1 without colours)
};

__device__ __forceinline__ void shf_corner_ids(const AttrMaps& m, int fn, int* ids) {
    const bool back = fn >= m.Ft;
    const int32_t* t = m.tri + (size_t)(back ? fn - m.Ft : fn) * 3;
    ids[0] = back ? t[2] : t[0];
    ids[1] = t[1];
    ids[2] = back ? t[0] : t[2];
}

// (u_0 x_0[k] + u_1 x_1[k]) + u_2 x_2[k] of a [V,3] array at the pixel's corners
__device__ __forceinline__ void shf_mix(const float* __restrict__ x, const int* ids, const float* u, float* out) {
    const float* x0 = x + (size_t)ids[0] * 3;
    const float* x1 = x + (size_t)ids[1] * 3;
    const float* x2 = x + (size_t)ids[2] * 3;
#pragma unroll
    for (int k = 0; k < 3; k++) out[k] = (u[0] * x0[k] + u[1] * x1[k]) + u[2] * x2[k];
}

// internal pixel q (index into the batch's maps) of view b, owned by fn
__device__ __forceinline__ void shf_pixel(const AttrMaps& m, const ShfInputs& in, int b, size_t q, int fn, ShfPixel& px) {
    float z[3], mm[3];
    fr_corner_depths(m, b, fn, z);
    va_weights(m, q, z, px.u);
    shf_corner_ids(m, fn, px.ids);
    shf_mix(in.normals + (size_t)(in.nb > 1 ? b : 0) * in.V * 3, px.ids, px.u, mm);
    px.r = sqrtf((mm[0] * mm[0] + mm[1] * mm[1]) + mm[2] * mm[2]);
    const float d = fmaxf(px.r, SS_EPS);
#pragma unroll
    for (int k = 0; k < 3; k++) px.n[k] = mm[k] / d;
    ss_basis(px.n, px.H);
    if (in.colors) {
        shf_mix(in.colors + (size_t)(in.cb > 1 ? b : 0) * in.V * 3, px.ids, px.u, px.a);
    } else {
        px.a[0] = px.a[1] = px.a[2] = 1.0f;
    }
}

// gm = dL/dm of the pixel from gn = dL/dn (THE ADJOINT above; d3m_sh_uv_fragments.h calls it too)
__device__ __forceinline__ void shf_normal_gradient(const ShfPixel& px, const float* gn, float* gm) {
    if (px.r >= SS_EPS) {
        const float dot = (px.n[0] * gn[0] + px.n[1] * gn[1]) + px.n[2] * gn[2];
#pragma unroll
        for (int k = 0; k < 3; k++) gm[k] = (gn[k] - px.n[k] * dot) / px.r;
    } else {
#pragma unroll
        for (int k = 0; k < 3; k++) gm[k] = gn[k] / SS_EPS;
    }
}

// ---- forward: fr_output_pixel_walk (d3m_fragments.h) with C = 3; a covered pixel's three values are formed in the gather -----
__global__ void __launch_bounds__(256) k_sh_fragment_images(AttrMaps m, ShfInputs in, const float* __restrict__ background,
                                                           float* __restrict__ images, float* __restrict__ alpha) {
    float val[4][3];
    fr_output_pixel_walk(
        m, 3, background, images, alpha,
        [&](int j, int b, size_t q, int fn) {
            ShfPixel px;
            shf_pixel(m, in, b, q, fn, px);
            const float* shp = in.sh + (size_t)(in.sb > 1 ? b : 0) * SHF_SUMS;
#pragma unroll
            for (int k = 0; k < 3; k++) {
                const float s = ss_light(shp + 9 * k, px.H);
                val[j][k] = in.colors ? px.a[k] * s : s;
            }
        },
        [&](int j, int k) { return val[j][k]; });
}

// ---- backward, per pixel: grid (parts, B), SET_BLOCK lanes; lane t of part p walks the view's internal pixels SET_BLOCK p + t,
// + SET_BLOCK parts, ... (step 1 of d3m_set_sums.h).  Each output may be NULL (not wanted): Qn / Qc the gradient image's normal
// and colour planes (view stride q_view floats), h [B,S,S,3], sh_partial [B, parts, 27].
__global__ void __launch_bounds__(SET_BLOCK) k_sh_fragment_backward_pixels(AttrMaps m, ShfInputs in,
                                                                           const float* __restrict__ grad_images,
                                                                           float* __restrict__ Qn, float* __restrict__ Qc,
                                                                           size_t q_view, float* __restrict__ h,
                                                                           float* __restrict__ sh_partial) {
    __shared__ float s_wave[SET_BLOCK / 64][SHF_SUMS];
    const int b = blockIdx.y, parts = gridDim.x, S = m.S, s = fr_output_size(m);
    const long S2 = (long)S * S;
    const float* shp = in.sh + (size_t)(in.sb > 1 ? b : 0) * SHF_SUMS;
    const float* g_view = grad_images + (size_t)b * 3 * s * s;
    float acc[SHF_SUMS];
#pragma unroll
    for (int j = 0; j < SHF_SUMS; j++) acc[j] = 0.0f;
    for (long i = (long)blockIdx.x * SET_BLOCK + threadIdx.x; i < S2; i += (long)parts * SET_BLOCK) {
        const size_t q = (size_t)b * S2 + i;
        const int fn = m.face_index_map[q];
        float hc[3] = {0.0f, 0.0f, 0.0f};
        if ((unsigned)fn < (unsigned)m.Fp) {
            const int y = (int)(i / S), x = (int)(i - (long)y * S);
            ShfPixel px;
            shf_pixel(m, in, b, q, fn, px);
            float sg[VA_CHUNK];
            va_pixel_grads(m, g_view, 3, 0, x, y, sg);
            float ga[3], gn[3] = {0.0f, 0.0f, 0.0f};
#pragma unroll
            for (int k = 0; k < 3; k++) {
                ga[k] = sg[k] * ss_light(shp + 9 * k, px.H);
                const float gs = in.colors ? sg[k] * px.a[k] : sg[k];
                if (sh_partial) {
#pragma unroll
                    for (int j = 0; j < 9; j++) acc[9 * k + j] += gs * px.H[j];
                }
                float d[3];
                ss_light_gradient(shp + 9 * k, px.n, d);
                gn[0] += gs * d[0]; gn[1] += gs * d[1]; gn[2] += gs * d[2];
            }
            float gm[3];
            shf_normal_gradient(px, gn, gm);
            const size_t at = (size_t)b * q_view + (size_t)(S - 1 - y) * S + x;       // output orientation: rows reversed
            if (Qn) {
#pragma unroll
                for (int k = 0; k < 3; k++) Qn[at + (size_t)k * S2] = gm[k];
            }
            if (Qc) {
#pragma unroll
                for (int k = 0; k < 3; k++) Qc[at + (size_t)k * S2] = ga[k];
            }
            if (h) {
                const float* nrm = in.normals + (size_t)(in.nb > 1 ? b : 0) * in.V * 3;
                const float* col = in.colors ? in.colors + (size_t)(in.cb > 1 ? b : 0) * in.V * 3 : nullptr;
#pragma unroll
                for (int c = 0; c < 3; c++) {
                    const float* nc = nrm + (size_t)px.ids[c] * 3;
                    hc[c] = (gm[0] * nc[0] + gm[1] * nc[1]) + gm[2] * nc[2];
                    if (col) {
                        const float* cc = col + (size_t)px.ids[c] * 3;
                        hc[c] += (ga[0] * cc[0] + ga[1] * cc[1]) + ga[2] * cc[2];
                    }
                }
            }
        }
        if (h) {
#pragma unroll
            for (int c = 0; c < 3; c++) h[3 * q + c] = hc[c];
        }
    }
    if (sh_partial)                                         // (uniform: the barrier is met by every lane)
        set_store_partial<SHF_SUMS, SHF_TREE>(acc, s_wave, sh_partial, b, parts);
}

// One lane per element of grad_sh [sb, 3, 9]: step 4 of d3m_set_sums.h, then -- a shared sh -- the views in ascending order.
__global__ void __launch_bounds__(SET_BLOCK) k_sh_fragment_finish(const float* __restrict__ sh_partial, int parts,
                                                                  float* __restrict__ grad_sh, int sb, int B) {
    const int i = blockIdx.x * SET_BLOCK + threadIdx.x;
    if (i >= sb * SHF_SUMS) return;
    const int q = i % SHF_SUMS;
    const int b_begin = sb > 1 ? i / SHF_SUMS : 0, b_end = sb > 1 ? b_begin + 1 : B;
    float total = 0.0f;
    for (int b = b_begin; b < b_end; b++) {
        float s[1];
        set_add_parts<1, SHF_SUMS>(sh_partial + q, b, parts, s);
        total = b == b_begin ? s[0] : total + s[0];
    }
    grad_sh[i] = total;
}

}  // namespace d3m
