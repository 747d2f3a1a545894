// d3m_sh_uv_fragments.h -- per-pixel spherical-harmonic shading of a UV albedo texture over a coverage record (AttrMaps,
// d3m_fragments.h): the albedo image [H, W, 3] looked up bilinearly at every internal pixel's interpolated uv (d3m_uv_texture.h),
// times the 9-term light of the per-pixel normalised interpolated normal (d3m_sh_fragments.h), the product formed at every
// INTERNAL pixel before the pooling; and the adjoint with respect to the image, the normals, the light and -- through the
// shared adjoint of d3m_fragment_geometry.h -- the screen vertices (neural_renderer/sh_uv_fragments.py).  Nothing of the two
// nodes it joins is restated here: their device functions are called.
//
// THE FUNCTION.  Internal pixel p of view b with owner fn >= 0:
//   u_c, the corner ids, m, r, n = m / max(r, 1e-6), H_j(n)     shf_pixel (d3m_sh_fragments.h), without colours
//   s_k = sum_j sh[b,k,j] H_j(n)                                ss_light
//   pos, the four taps and their weights w_j                    uvt_pixel_taps (d3m_uv_texture.h): corners wrapped per corner, a
//                                                               fill_back copy reads corners 2 - c
//   a_k = sum_j image[tap_j][k] * w_j, in tap order, from 0     value_k = a_k * s_k
// The normal is NOT flipped for a pixel a back copy owns.  An uncovered pixel takes background[k] (NULL: 0).  The image is what
// fr_output_pixel_walk makes of that map: rows reversed and, with anti-aliasing, ((p00 + p01) + p10) + p11 in OUTPUT
// orientation, times 1/4, AFTER the product, background included.  alpha: the bits of k_vertex_attribute_images' alpha.
//
// THE ADJOINT, for g = dL/dimages and sg_k = scale g[b,k,out(p)] (scale = 1 or 1/4: va_pixel_grads).  Per covered internal
// pixel, everything recomputed from the record and the inputs (nothing is kept from the forward):
//   ga_k = sg_k s_k   (dL/da_k)          gs_k = sg_k a_k   (dL/ds_k)
//   gn, gm            as in d3m_sh_fragments.h (shf_normal_gradient: the one statement both nodes call)
//   Dx = sum over k = 0, 1, 2, from 0, of ga_k * dax_k,  Dy likewise with day_k      dax_k, day_k: the bilinear lookup's slopes
//                     along pos_x, pos_y at the forward's pos (FgUvSlopes, d3m_fragment_geometry.h: the statement that
//                     k_uv_texture_pixel_grads calls too); Dx (Dy) = 0 where pos_x (pos_y) sits at a clamp limit
//   h_c = ((gm_x n_c.x + gm_y n_c.y) + gm_z n_c.z) + ((W - 1) cx_c Dx + (H - 1) cy_c Dy)           (dL/du_c)
// THE ASSOCIATION of h_c's second sum: the channels are summed FIRST (Dx, Dy above, k ascending), then the two axes -- sum_k
// ga_k (dax_k (W-1) cx_c + day_k (H-1) cy_c) with the factors that do not depend on k taken out of the sum, which is the order
// k_uv_texture_pixel_grads has for its own h.
// THE ORDER of every sum, the same bits on every run (no float atomics anywhere):
//   sh       as d3m_sh_fragments.h: 27 sums per view of gs_k H_j(n) through the tree of d3m_set_sums.h with SHF_PER_PART,
//            SHF_MAX_PARTS, SHF_TREE; k_sh_fragment_finish is its step 4 and sums a shared sh over the views in ascending order.
//   normals  gm goes into a gradient image Qn [B,3,S,S] at the internal size, in output orientation, written at covered pixels
//            only and read at owned pixels only by the attribute adjoint's gather over the record re-labelled image_size = S,
//            anti_aliasing = 0 (d3m_sh_fragments.h, the SAME kernels).
//   image    ga goes into a second gradient image Qa [B,3,S,S], same size and orientation, and is fed to
//            k_uv_texture_images_clear_max, k_uv_texture_images_scatter and k_uv_texture_images_convert (d3m_uv_texture.h, the
//            SAME kernels) over the same re-labelled record, scale 1: term = w_j * ga_k, gmax = max |Qa| so |t| <= gmax holds,
//            frac = 62 - ceil(log2(B S S)).  The clear/max kernel reads EVERY element of Qa, so the per-pixel kernel WRITES +0
//            AT THE UNCOVERED PIXELS of Qa (the choice taken here; the maximum is not restricted): no element of the caller's
//            scratch is read before it is written.  The zero, Inf / NaN and untouched-texel (+0) rules are d3m_uv_texture.h's.
//   screen vertices    h [B,S,S,3] (every element written, +0 where uncovered; the same per-pixel launch writes it) goes to
//            d3m_fragment_geometry_backward.
//
// Launches.  Forward: k_sh_uv_fragment_images.  Backward: k_sh_uv_fragment_backward_pixels; k_sh_fragment_finish (grad_sh
// only); the normals' gather (k_vertex_attribute_face_sums, k_vertex_attribute_large_face_sums,
// k_vertex_attribute_adjoint_rows, with k_vertex_attribute_adjoint_chunks on a mesh with long rows); the image's three.
#pragma once
#include "d3m_fragment_geometry.h"
#include "d3m_sh_fragments.h"
#include "d3m_uv_texture.h"

namespace d3m {

// a_k of a pixel's taps: the four products added in tap order from 0, one channel at a time (three texel registers, not twelve)
__device__ __forceinline__ float shuv_albedo(const float* __restrict__ img, const UvtTaps& t, int k) {
    float v = 0.0f;
#pragma unroll
    for (int j = 0; j < 4; j++) v += img[(size_t)t.pix[j] * 3 + k] * t.w[j];
    return v;
}

// ---- forward: fr_output_pixel_walk (d3m_fragments.h) with C = 3; a covered pixel's three values are formed in the gather -----
__global__ void __launch_bounds__(256) k_sh_uv_fragment_images(AttrMaps m, ShfInputs in, UvTexture tx,
                                                              const float* __restrict__ image,
                                                              const float* __restrict__ background,
                                                              float* __restrict__ images, float* __restrict__ alpha) {
    const float* img = image + (size_t)(tx.image_batch > 1 ? (int)blockIdx.y : 0) * tx.H * tx.W * 3;
    float val[4][3];
    fr_output_pixel_walk(
        m, 3, background, images, alpha,
        [&](int j, int b, size_t q, int fn) {
            ShfPixel px;
            shf_pixel(m, in, b, q, fn, px);
            UvtTaps taps;
            uvt_pixel_taps(m, tx, b, q, fn, taps);
            const float* shp = in.sh + (size_t)(in.sb > 1 ? b : 0) * SHF_SUMS;
#pragma unroll
            for (int k = 0; k < 3; k++) val[j][k] = shuv_albedo(img, taps, k) * ss_light(shp + 9 * k, px.H);
        },
        [&](int j, int k) { return val[j][k]; });
}

// ---- backward, per pixel: the grid and the walk of k_sh_fragment_backward_pixels.  Each output may be NULL (not wanted): Qn
// [B,3,S,S] (covered pixels only), Qa [B,3,S,S] (EVERY pixel), h [B,S,S,3] (every pixel), sh_partial [B, parts, 27].
__global__ void __launch_bounds__(SET_BLOCK) k_sh_uv_fragment_backward_pixels(AttrMaps m, ShfInputs in, UvTexture tx,
                                                                              const float* __restrict__ image,
                                                                              const float* __restrict__ grad_images,
                                                                              float* __restrict__ Qn, float* __restrict__ Qa,
                                                                              float* __restrict__ h,
                                                                              float* __restrict__ sh_partial) {
    __shared__ float s_wave[SET_BLOCK / 64][SHF_SUMS];
    const int b = blockIdx.y, parts = gridDim.x, S = m.S, s = fr_output_size(m);
    const long S2 = (long)S * S;
    const float* shp = in.sh + (size_t)(in.sb > 1 ? b : 0) * SHF_SUMS;
    const float* g_view = grad_images + (size_t)b * 3 * s * s;
    const float* img = image + (size_t)(tx.image_batch > 1 ? b : 0) * tx.H * tx.W * 3;
    const float* nrm = in.normals + (size_t)(in.nb > 1 ? b : 0) * in.V * 3;
    float acc[SHF_SUMS];
#pragma unroll
    for (int j = 0; j < SHF_SUMS; j++) acc[j] = 0.0f;
    for (long i = (long)blockIdx.x * SET_BLOCK + threadIdx.x; i < S2; i += (long)parts * SET_BLOCK) {
        const size_t q = (size_t)b * S2 + i;
        const int fn = m.face_index_map[q];
        const int y = (int)(i / S), x = (int)(i - (long)y * S);
        const size_t at = ((size_t)b * 3 * S + (size_t)(S - 1 - y)) * S + x;          // output orientation: rows reversed
        float hc[3] = {0.0f, 0.0f, 0.0f}, ga[3] = {0.0f, 0.0f, 0.0f};
        if ((unsigned)fn < (unsigned)m.Fp) {
            ShfPixel px;
            shf_pixel(m, in, b, q, fn, px);
            float z[3], pos_x, pos_y;
            fr_corner_depths(m, b, fn, z);
            UvtCorners kc;
            uvt_pixel_position(m, tx, q, fn, z, kc, pos_x, pos_y);
            const FgUvSlopes sl = fg_uv_slopes(tx, img, pos_x, pos_y);
            UvtTaps taps;
            uvt_pixel_taps(m, tx, b, q, fn, taps);
            float sg[VA_CHUNK];
            va_pixel_grads(m, g_view, 3, 0, x, y, sg);
            float gn[3] = {0.0f, 0.0f, 0.0f}, dx = 0.0f, dy = 0.0f;
#pragma unroll
            for (int k = 0; k < 3; k++) {
                ga[k] = sg[k] * ss_light(shp + 9 * k, px.H);
                const float gs = sg[k] * shuv_albedo(img, taps, k);
                if (sh_partial) {
#pragma unroll
                    for (int j = 0; j < 9; j++) acc[9 * k + j] += gs * px.H[j];
                }
                float d[3];
                ss_light_gradient(shp + 9 * k, px.n, d);
                gn[0] += gs * d[0]; gn[1] += gs * d[1]; gn[2] += gs * d[2];
                if (h) sl.add(k, ga[k], dx, dy);
            }
            float gm[3];
            shf_normal_gradient(px, gn, gm);
            if (Qn) {
#pragma unroll
                for (int k = 0; k < 3; k++) Qn[at + (size_t)k * S2] = gm[k];
            }
            if (h) {
                sl.finish(kc, dx, dy, hc);
#pragma unroll
                for (int c = 0; c < 3; c++) {
                    const float* nc = nrm + (size_t)px.ids[c] * 3;
                    hc[c] = ((gm[0] * nc[0] + gm[1] * nc[1]) + gm[2] * nc[2]) + hc[c];
                }
            }
        }
        if (Qa) {
#pragma unroll
            for (int k = 0; k < 3; k++) Qa[at + (size_t)k * S2] = ga[k];
        }
        if (h) {
#pragma unroll
            for (int c = 0; c < 3; c++) h[3 * q + c] = hc[c];
        }
    }
    if (sh_partial)                                         // (uniform: the barrier is met by every lane)
        set_store_partial<SHF_SUMS, SHF_TREE>(acc, s_wave, sh_partial, b, parts);
}

}  // namespace d3m
