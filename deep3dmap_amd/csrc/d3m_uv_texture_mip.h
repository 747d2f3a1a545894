// d3m_uv_texture_mip.h -- mip-mapped per-pixel uv texture images: the node of d3m_uv_texture.h with a level of detail per
// pixel, a box pyramid of the image, a trilinear (eight-tap) lookup and an adjoint that goes back down the pyramid.  Four
// bilinear taps are right when the texture is magnified; when one pixel spans many texels they alias and leave most of the
// footprint with a gradient of exactly +0.  faces_uv stays a constant.
//
// PYRAMID.  Levels 0..L, 1 <= L <= UVT_MAX_LEVEL, H and W divisible by 2^L.  Level 0 is the image; level l + 1 has H >> (l + 1)
// rows and W >> (l + 1) columns and texel (y, x) of it is (((a00 + a01) + a10) + a11) * 0.25 of level l's (2y, 2x), (2y, 2x + 1),
// (2y + 1, 2x), (2y + 1, 2x + 1): a recursive definition in a fixed order, so the bits do not depend on the launches.  All
// levels live in one buffer [n_img, T, C], T = sum_l (H >> l)(W >> l), level l at texel offset[l] (the host computes them).
//
// LEVEL OF DETAIL of internal pixel p owned by fn.  pos_x, pos_y: uvt_pixel_position (d3m_uv_texture.h), the bits of the
// bilinear node.  finv = face_inverse(face, S): a_c = finv[3c], b_c = finv[3c + 1] are the x and y slopes of the pixel-space
// affine barycentric of corner c; z_c the corner depths, d = depth_map[p], u_c the va_weights, (cx_c, cy_c) the wrapped uv:
//   A = (a_0/z_0 + a_1/z_1) + a_2/z_2, B likewise with b_c;
//   du_c/dx = d (a_c/z_c - u_c A), du_c/dy = d (b_c/z_c - u_c B)            (the derivative of w_c/z_c / sum_k w_k/z_k);
//   px_x = ((du_0/dx cx_0 + du_1/dx cx_1) + du_2/dx cx_2) (W - 1), py_x with cy_c and (H - 1), px_y and py_y with d/dy;
//   rho2 = fmaxf(px_x^2 + py_x^2, px_y^2 + py_y^2), lambda = 0.5 log2f(rho2) + lod_bias,
//   lambda_c = fminf(fmaxf(lambda, 0), L): a NaN and -inf (a constant uv: rho2 = 0) go to 0, as the position clamp sends a NaN
//   to 0.  With anti-aliasing the level is that of the internal pixel; the 2 x 2 pooling follows.
//
// LOOKUP.  l0 = min((int)lambda_c, L - 1), l1 = l0 + 1, t = lambda_c - l0 (exact; lambda_c = L gives l0 = L - 1, t = 1).  At
// level l: pos^l_x = clamp((pos_x + 0.5) 2^-l - 0.5, 0, (W >> l) - 1), y likewise -- a texel of level l sits at the centre of the
// level-0 block it averages, so an affine image is reproduced away from the clamp --, then bilinear_taps on the level's size.
// At level 0 that is pos itself and pos is taken (the sum with 0.5 and its difference would round twice for nothing), so level
// 0's taps are the bilinear node's, bit for bit.
//   value[k] = (1 - t) v_l0[k] + t v_l1[k], each v the four products added in tap order from 0;
// a level whose weight is exactly 0 is not read (its v is 0).  Background, row reversal, pooling and alpha: k_uv_texture_images.
// The value is continuous in pos and in lambda: at an integer lambda both sides agree.  lambda_c = 0 gives the bits of
// k_uv_texture_images.
//
// THE ADJOINT with respect to the image: the number format of d3m_uv_texture.h, extended to the pyramid.
//   term     ((lw w_j) (scale g)) in f32, lw = 1 - t or t; a term whose weight lw w_j is 0 is skipped;
//   add      __double2ll_rn((double)term 2^(frac - E)) with a 64-bit INTEGER atomic into one int64 accumulator per element of
//            EVERY level: the scratch is 8 n_img T C bytes plus the block maxima.  The eight weights of a pixel sum to 1, so
//            frac = 62 - ceil(log2(B S S)) and the overflow argument are those of d3m_uv_texture.h; clear and gmax are its
//            k_uv_texture_images_clear_max;
//   convert  is also the pyramid's adjoint, as a gather: grad[y, x, k] = (float)(sum over l = 0..L, ascending, of
//            (double)acc_l[y >> l][x >> l][k] 2^(E - frac - 2l)), summed in double in that order.
// Integer sums are associative and the final sum has a fixed order: the same bits on every run, for every arrival order and
// launch shape; no float atomics.  gmax == 0: every element an exact +0; gmax not finite: every element NaN; a texel under no
// footprint: +0.  Launches: forward at most 3 (k_texture_mip_tile, k_texture_mip_tail when L > UVT_TILE_LEVELS,
// k_uv_texture_mip_images); backward 3 (k_uv_texture_images_clear_max, k_uv_texture_mip_images_scatter,
// k_uv_texture_mip_images_convert).  The pyramid is transient: the backward reads the record, faces_uv and the sizes only.
#pragma once
#include "d3m_uv_texture.h"

namespace d3m {

constexpr int UVT_MAX_LEVEL = 15;
constexpr int UVT_TILE = 32;             // k_texture_mip_tile: a 32 x 32 level-0 tile goes through LDS ...
constexpr int UVT_TILE_LEVELS = 5;       // ... up to level 5 (one texel)
constexpr int UVT_TILE_TEXELS = 1024 + 256 + 64 + 16 + 4 + 1;
constexpr int UVT_TAIL_BLOCK = 1024;

struct UvMip {
    int L;
    float lod_bias;
    long T;                              // texels of all levels of one image
    long offset[UVT_MAX_LEVEL + 1];      // of level l's first texel
};

// ---- pyramid ------------------------------------------------------------------------------------------------------------
// One workgroup per 32 x 32 level-0 tile (clipped to the image; H and W are multiples of 2^min(L, 5), so every level of the
// tile is whole) and image; the channels in chunks of UVT_CHUNK.  Lanes run along the tile rows' contiguous (x, c) axis.  Level
// 0 is copied into the pyramid, levels 1..min(L, 5) are built in LDS and stored.
__global__ void __launch_bounds__(256) k_texture_mip_tile(const float* __restrict__ image, UvMip mp, int H, int W, int C,
                                                         float* __restrict__ pyramid) {
    __shared__ float s_tile[UVT_TILE_TEXELS * UVT_CHUNK];
    const int tiles_x = (W + UVT_TILE - 1) / UVT_TILE;
    const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x, n = blockIdx.y;
    const int x0 = tx * UVT_TILE, y0 = ty * UVT_TILE;
    const int tw = min(UVT_TILE, W - x0), th = min(UVT_TILE, H - y0);
    const int lt = min(mp.L, UVT_TILE_LEVELS);
    const float* img = image + (size_t)n * H * W * C;
    float* pyr = pyramid + (size_t)n * mp.T * C;
    for (int k0 = 0; k0 < C; k0 += UVT_CHUNK) {
        const int cc = min(UVT_CHUNK, C - k0), row = tw * cc;
        for (int e = threadIdx.x; e < th * row; e += 256) {
            const int y = e / row, r = e - y * row, x = r / cc, k = r - x * cc;
            const size_t at = ((size_t)(y0 + y) * W + x0 + x) * C + k0 + k;
            const float v = img[at];
            s_tile[e] = v;
            pyr[at] = v;
        }
        __syncthreads();
        int base = 0;                                                   // level l - 1's first texel in s_tile
        for (int l = 1; l <= lt; l++) {
            const int wp = tw >> (l - 1), wl = tw >> l, hl = th >> l, next = base + (th >> (l - 1)) * wp;
            float* dst = pyr + (size_t)mp.offset[l] * C;
            const int Wl = W >> l;
            for (int e = threadIdx.x; e < hl * wl * cc; e += 256) {
                const int y = e / (wl * cc), r = e - y * wl * cc, x = r / cc, k = r - x * cc;
                const float* a = s_tile + (base + 2 * y * wp + 2 * x) * cc + k;
                const float v = (((a[0] + a[cc]) + a[wp * cc]) + a[(wp + 1) * cc]) * 0.25f;
                s_tile[(next + y * wl + x) * cc + k] = v;
                dst[((size_t)((y0 >> l) + y) * Wl + (x0 >> l) + x) * C + k0 + k] = v;
            }
            __syncthreads();
            base = next;
        }
    }
}

// Levels UVT_TILE_LEVELS + 1 .. L, each from the one below it in the pyramid: one workgroup per image walks the levels (level
// 6 of a 2048 x 2048 image has 32 x 32 texels), lanes along the contiguous (x, c) axis.
__global__ void __launch_bounds__(UVT_TAIL_BLOCK) k_texture_mip_tail(UvMip mp, int H, int W, int C, float* pyramid) {
    float* pyr = pyramid + (size_t)blockIdx.x * mp.T * C;
    for (int l = UVT_TILE_LEVELS + 1; l <= mp.L; l++) {
        const int wl = W >> l, hl = H >> l, wp = W >> (l - 1);
        const float* src = pyr + (size_t)mp.offset[l - 1] * C;
        float* dst = pyr + (size_t)mp.offset[l] * C;
        const long row = (long)wl * C, n = (long)hl * row;
        for (long e = threadIdx.x; e < n; e += UVT_TAIL_BLOCK) {
            const int y = (int)(e / row), r = (int)(e - (long)y * row), x = r / C, k = r - x * C;
            const float* a = src + ((size_t)2 * y * wp + 2 * x) * C + k;
            dst[e] = (((a[0] + a[C]) + a[(size_t)wp * C]) + a[((size_t)wp + 1) * C]) * 0.25f;
        }
        __threadfence();                                                // the next level reads what other lanes stored
        __syncthreads();
    }
}

// ---- level of detail and taps ---------------------------------------------------------------------------------------------
// lambda_c of internal pixel q owned by the face whose nine screen-space floats are `face`; k: its corners (uvt_pixel_position)
__device__ __forceinline__ float uvt_pixel_lod(const AttrMaps& m, const UvTexture& tx, const UvMip& mp, size_t q,
                                               const float* face, const UvtCorners& k) {
    float finv[9];
    face_inverse(face, m.S, finv);
    const float d = m.depth_map[q];
    float az[3], bz[3];
#pragma unroll
    for (int c = 0; c < 3; c++) {
        az[c] = finv[3 * c] / face[3 * c + 2];
        bz[c] = finv[3 * c + 1] / face[3 * c + 2];
    }
    const float A = (az[0] + az[1]) + az[2], B = (bz[0] + bz[1]) + bz[2];
    float ux[3], uy[3];
#pragma unroll
    for (int c = 0; c < 3; c++) {
        ux[c] = d * (az[c] - k.u[c] * A);
        uy[c] = d * (bz[c] - k.u[c] * B);
    }
    const float x_max = (float)(tx.W - 1), y_max = (float)(tx.H - 1);
    const float px_x = ((ux[0] * k.cx[0] + ux[1] * k.cx[1]) + ux[2] * k.cx[2]) * x_max;
    const float py_x = ((ux[0] * k.cy[0] + ux[1] * k.cy[1]) + ux[2] * k.cy[2]) * y_max;
    const float px_y = ((uy[0] * k.cx[0] + uy[1] * k.cx[1]) + uy[2] * k.cx[2]) * x_max;
    const float py_y = ((uy[0] * k.cy[0] + uy[1] * k.cy[1]) + uy[2] * k.cy[2]) * y_max;
    const float rho2 = fmaxf(px_x * px_x + py_x * py_x, px_y * px_y + py_y * py_y);
    const float lambda = 0.5f * log2f(rho2) + mp.lod_bias;
    return fminf(fmaxf(lambda, 0.0f), (float)mp.L);
}

struct UvtMipTaps {
    int pix[8];                          // texel index in the pyramid of one image: offset[l] + y (W >> l) + x; l0's four, l1's
    float w[8];
    float lw[2];                         // 1 - t, t
};

// the eight taps of internal pixel q of view b, owned by fn; returns lambda_c
__device__ __forceinline__ float uvt_mip_pixel_taps(const AttrMaps& m, const UvTexture& tx, const UvMip& mp, int b, size_t q,
                                                    int fn, UvtMipTaps& t) {
    float face[9], z[3];
    const float* fp = m.faces + ((size_t)b * m.Fp + fn) * 9;
#pragma unroll
    for (int i = 0; i < 9; i++) face[i] = fp[i];
    fr_corner_depths(face, z);
    UvtCorners k;
    float pos_x, pos_y;
    uvt_pixel_position(m, tx, q, fn, z, k, pos_x, pos_y);
    const float lambda = uvt_pixel_lod(m, tx, mp, q, face, k);
    const int l0 = min((int)lambda, mp.L - 1);
    const float frac = lambda - (float)l0;
    t.lw[0] = 1 - frac;
    t.lw[1] = frac;
#pragma unroll
    for (int h = 0; h < 2; h++) {
        const int l = l0 + h, Hl = tx.H >> l, Wl = tx.W >> l;
        const float down = __uint_as_float((unsigned)(127 - l) << 23);                  // 2^-l
        const float lx = l == 0 ? pos_x : fminf(fmaxf((pos_x + 0.5f) * down - 0.5f, 0.0f), (float)(Wl - 1));
        const float ly = l == 0 ? pos_y : fminf(fmaxf((pos_y + 0.5f) * down - 0.5f, 0.0f), (float)(Hl - 1));
        TexelTaps tt;
        bilinear_taps(lx, ly, Hl, Wl, tt);
        const long first = mp.offset[l];
#pragma unroll
        for (int j = 0; j < 4; j++) {
            t.pix[4 * h + j] = (int)(first + tt.pix[j]);
            t.w[4 * h + j] = tt.w[j];
        }
    }
    return lambda;
}

// lambda_c [B, S, S] in map orientation, 0 where uncovered: one lane per internal pixel
__global__ void __launch_bounds__(256) k_uv_texture_lod(AttrMaps m, UvTexture tx, UvMip mp, float* __restrict__ lod) {
    const long p = (long)blockIdx.x * 256 + threadIdx.x;
    int b, x, y, fn;
    if (!fr_pixel(m, p, b, x, y, fn)) return;
    float lambda = 0.0f;
    if (fn >= 0) {
        UvtMipTaps t;
        lambda = uvt_mip_pixel_taps(m, tx, mp, b, (size_t)p, fn, t);
    }
    lod[p] = lambda;
}

// ---- forward: fr_output_pixel_walk (d3m_fragments.h) with eight taps per internal pixel -------------------------------------
__global__ void __launch_bounds__(256) k_uv_texture_mip_images(AttrMaps m, UvTexture tx, UvMip mp,
                                                              const float* __restrict__ pyramid,
                                                              const float* __restrict__ background, float* __restrict__ images,
                                                              float* __restrict__ alpha) {
    const int C = tx.C;
    const float* img = pyramid + (size_t)(tx.image_batch > 1 ? (int)blockIdx.y : 0) * mp.T * C;
    UvtMipTaps taps[4];
    fr_output_pixel_walk(
        m, C, background, images, alpha,
        [&](int j, int b, size_t q, int fn) { uvt_mip_pixel_taps(m, tx, mp, b, q, fn, taps[j]); },
        [&](int j, int k) {
            float v[2] = {0.0f, 0.0f};
#pragma unroll
            for (int h = 0; h < 2; h++) {
                if (taps[j].lw[h] == 0.0f) continue;                    // not read
#pragma unroll
                for (int a = 0; a < 4; a++) v[h] += img[(size_t)taps[j].pix[4 * h + a] * C + k] * taps[j].w[4 * h + a];
            }
            return taps[j].lw[0] * v[0] + taps[j].lw[1] * v[1];
        });
}

// ---- adjoint --------------------------------------------------------------------------------------------------------------
// 2. uvt_scatter_taps (d3m_uv_texture.h) with eight taps of weight lw * w_j, over the accumulators of every level
__global__ void __launch_bounds__(256) k_uv_texture_mip_images_scatter(AttrMaps m, UvTexture tx, UvMip mp,
                                                                      const float* __restrict__ grad_images,
                                                                      const unsigned* __restrict__ block_max, int n_max,
                                                                      int frac, unsigned long long* __restrict__ acc) {
    uvt_scatter_taps<8>(m, tx.C, tx.image_batch, (size_t)mp.T * tx.C, grad_images, block_max, n_max, frac, acc,
                        [&](int b, size_t q, int fn, int* pix, float* w) {
                            UvtMipTaps t;
                            uvt_mip_pixel_taps(m, tx, mp, b, q, fn, t);
#pragma unroll
                            for (int j = 0; j < 8; j++) {
                                pix[j] = t.pix[j];
                                w[j] = t.lw[j >> 2] * t.w[j];
                            }
                        });
}

// 3. one lane per element of grad_image (a fixed grid striding over them): the element's accumulator and its ancestors', in
// level order; neighbouring lanes share the ancestors.  Every element is written.
__global__ void __launch_bounds__(256) k_uv_texture_mip_images_convert(const long long* __restrict__ acc, UvMip mp, int n_img,
                                                                      int H, int W, int C,
                                                                      const unsigned* __restrict__ block_max, int n_max,
                                                                      int frac, float* __restrict__ grad_image) {
    const UvtQuantum qn = uvt_quantum(uvt_gmax_bits(block_max, n_max), frac);
    const long per_row = (long)W * C, per_image = (long)H * per_row, n = (long)n_img * per_image;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
        float v = 0.0f;
        if (qn.state == UVT_FINITE) {
            const int im = (int)(i / per_image);
            const long r = i - (long)im * per_image;
            const int y = (int)(r / per_row), rr = (int)(r - (long)y * per_row), x = rr / C, k = rr - x * C;
            const long long* a = acc + (size_t)im * mp.T * C + k;
            double sum = 0.0, down = qn.down;
            for (int l = 0; l <= mp.L; l++) {
                sum += (double)a[(size_t)(mp.offset[l] + (long)(y >> l) * (W >> l) + (x >> l)) * C] * down;
                down *= 0.25;                                           // 2^(E - frac - 2 l), exact
            }
            v = (float)sum;
        } else if (qn.state == UVT_NOT_FINITE) {
            v = __uint_as_float(0x7FC00000u);
        }
        grad_image[i] = v;
    }
}

}  // namespace d3m
