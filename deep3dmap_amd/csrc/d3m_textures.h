// d3m_textures.h -- texture asset kernels: uv image -> per-face texture cubes, and texture cubes -> atlas image.
// Replaces NR/cuda/load_textures_cuda_kernel.cu:23-114 (LTK) and create_texture_image_cuda_kernel.cu:10-115 (CTK).
// Both are element-wise and HBM-bound (one texel / one atlas pixel per lane, outputs written coalesced).
#pragma once
#include "d3m_launch.h"
#include "d3m_row_gather.h"

enum { D3M_WRAP_REPEAT = 0, D3M_WRAP_MIRRORED_REPEAT = 1, D3M_WRAP_CLAMP_TO_EDGE = 2, D3M_WRAP_CLAMP_TO_BORDER = 3 };

// LTK:6-14
__device__ __forceinline__ float tex_mod(float x, float y) { return x > 0 ? fmodf(x, y) : y + fmodf(x, y); }

// LTK:55-76, applied ONCE to a private copy of the uv coordinate.  The reference writes the wrapped value back
// into the shared `faces` array from every texel thread: a race that is harmless except at integer coordinates
// under REPEAT (0 -> 1 -> 0 ...), where its result depends on thread scheduling.  "Once" is what a thread that
// sees the caller's input computes; `faces` stays read-only here.
__device__ __forceinline__ float wrap_uv(float v, int wrapping) {
    if (wrapping == D3M_WRAP_REPEAT) return tex_mod(v, 1.0f);
    if (wrapping == D3M_WRAP_MIRRORED_REPEAT) return (tex_mod(v, 2.0f) < 1) ? tex_mod(v, 1.0f) : 1 - tex_mod(v, 1.0f);
    if (wrapping == D3M_WRAP_CLAMP_TO_EDGE) return fmaxf(fminf(v, 1.0f), 0.0f);
    return v;
}

// Barycentric direction of texel r of a ts^3 cube (LTK:42-50); the reference divides in double and stores f32.
// Texel 0 has direction (0,0,0): it is not normalised, so its position is (0,0) whatever the face -- pixel (0,0) with
// weight 1, the one pixel that every face reads.
__device__ __forceinline__ void texel_direction(int r, int ts, float& dim0, float& dim1, float& dim2) {
    dim0 = (float)((r / (ts * ts)) / (ts - 1.));
    dim1 = (float)(((r / ts) % ts) / (ts - 1.));
    dim2 = (float)((r % ts) / (ts - 1.));
    if (0 < dim0 + dim1 + dim2) {
        const float sum = dim0 + dim1 + dim2;
        dim0 /= sum; dim1 /= sum; dim2 /= sum;
    }
}

// The image taps of texel r of the face whose uv corners are face_uv[6] (not yet wrapped): the map image -> cubes is
// tex[k] = sum_j image[pix[j]][k] * w[j], accumulated in j order from 0 (bilinear: the four taps p00, p10, p01, p11 of
// LTK; on the last row / column two of them are the same pixel).  Nearest: one tap of weight 1, read as a copy.  Returns
// the number of taps; 0 under CLAMP_TO_BORDER (the reference writes zeros).  Pixel indices are y * W + x.
struct TexelTaps {
    long pix[4];
    float w[4];
};

// The four bilinear taps of the texture-space position (pos_x, pos_y), 0 <= pos_x <= W - 1 and 0 <= pos_y <= H - 1, in LTK's
// order p00, p10, p01, p11 (shared by texel_taps and by the per-pixel lookup of d3m_uv_texture.h).
__device__ __forceinline__ void bilinear_taps(float pos_x, float pos_y, int image_height, int image_width, TexelTaps& t) {
    const int xi = (int)pos_x, yi = (int)pos_y;
    const float wx1 = pos_x - (float)xi, wx0 = 1 - wx1, wy1 = pos_y - (float)yi, wy0 = 1 - wy1;
    // (int)(pos_y + 1), not yi + 1: the f32 sum can round up to the next integer (LTK)
    const int y1 = min((int)(pos_y + 1), image_height - 1), x1 = min(xi + 1, image_width - 1);
    t.pix[0] = (long)yi * image_width + xi; t.w[0] = wx0 * wy0;
    t.pix[1] = (long)y1 * image_width + xi; t.w[1] = wx0 * wy1;
    t.pix[2] = (long)yi * image_width + x1; t.w[2] = wx1 * wy0;
    t.pix[3] = (long)y1 * image_width + x1; t.w[3] = wx1 * wy1;
}

__device__ __forceinline__ int texel_taps(const float* __restrict__ face_uv, int r, int ts, int image_height,
                                          int image_width, int wrapping, int use_bilinear, TexelTaps& t) {
    if (wrapping == D3M_WRAP_CLAMP_TO_BORDER) return 0;        // LTK:97,109
    float dim0, dim1, dim2;
    texel_direction(r, ts, dim0, dim1, dim2);
    float uv[6];
#pragma unroll
    for (int k = 0; k < 6; k++) uv[k] = wrap_uv(face_uv[k], wrapping);
    const float pos_x = (uv[0] * dim0 + uv[2] * dim1 + uv[4] * dim2) * (float)(image_width - 1);
    const float pos_y = (uv[1] * dim0 + uv[3] * dim1 + uv[5] * dim2) * (float)(image_height - 1);
    if (use_bilinear) {
        bilinear_taps(pos_x, pos_y, image_height, image_width, t);
        return 4;
    }
    t.pix[0] = (long)(int)roundf(pos_y) * image_width + (int)roundf(pos_x);
    t.w[0] = 1.0f;
    return 1;
}

// One texel: tex[0..2] from image [H, W, 3] (the arithmetic of LTK, shared by every kernel that samples a uv image).
__device__ __forceinline__ void load_texel(const float* __restrict__ image, const float* __restrict__ face_uv, int r,
                                           int ts, int image_height, int image_width, int wrapping, int use_bilinear,
                                           float* __restrict__ tex) {
    TexelTaps t;
    const int n = texel_taps(face_uv, r, ts, image_height, image_width, wrapping, use_bilinear, t);
    if (n == 0) {
        tex[0] = 0; tex[1] = 0; tex[2] = 0;
    } else if (n == 4) {
        const float* p00 = image + t.pix[0] * 3;
        const float* p10 = image + t.pix[1] * 3;
        const float* p01 = image + t.pix[2] * 3;
        const float* p11 = image + t.pix[3] * 3;
#pragma unroll
        for (int k = 0; k < 3; k++) {
            float c = 0;
            c += p00[k] * t.w[0];
            c += p10[k] * t.w[1];
            c += p01[k] * t.w[2];
            c += p11[k] * t.w[3];
            tex[k] = c;
        }
    } else {
        const float* p = image + t.pix[0] * 3;
        tex[0] = p[0]; tex[1] = p[1]; tex[2] = p[2];
    }
}

// One lane per texel of textures [F, ts, ts, ts, 3]; faces with is_update == 0 are left untouched.
__global__ void __launch_bounds__(256) k_load_textures(const float* __restrict__ image,
                                                       const int32_t* __restrict__ is_update,
                                                       const float* __restrict__ faces, float* __restrict__ textures,
                                                       long n_texels, int ts, int image_height, int image_width,
                                                       int wrapping, int use_bilinear) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n_texels) return;
    const int ts3 = ts * ts * ts;
    const int fn = (int)(i / ts3);
    if (is_update[fn] == 0) return;
    const int r = (int)(i - (long)fn * ts3);
    load_texel(image, faces + (long)fn * 6, r, ts, image_height, image_width, wrapping, use_bilinear, textures + i * 3);
}

// ---- learnable uv images: image [B, H, W, 3] -> cubes [B, F, ts, ts, ts, 3] and its adjoint ----------------------------
// One lane per texel of every view into a FRESH output: faces with mask[f] == 0 (mask NULL: none) copy base (batch 1 or B;
// NULL: zeros), the others are load_texel of view b's image -- bit for bit what k_load_textures writes.
__global__ void __launch_bounds__(256) k_textures_from_image(const float* __restrict__ image,
                                                             const int32_t* __restrict__ mask,
                                                             const float* __restrict__ faces_uv,
                                                             const float* __restrict__ base, int base_batch,
                                                             float* __restrict__ textures, long n_texels, int ts,
                                                             int image_height, int image_width, int wrapping,
                                                             int use_bilinear) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    const int b = blockIdx.y;
    if (i >= n_texels) return;
    const int ts3 = ts * ts * ts;
    const int fn = (int)(i / ts3);
    float* tex = textures + ((long)b * n_texels + i) * 3;
    if (mask && mask[fn] == 0) {
        if (base) {
            const float* src = base + ((base_batch > 1 ? (long)b * n_texels : 0) + i) * 3;
            tex[0] = src[0]; tex[1] = src[1]; tex[2] = src[2];
        } else {
            tex[0] = 0; tex[1] = 0; tex[2] = 0;
        }
        return;
    }
    const int r = (int)(i - (long)fn * ts3);
    load_texel(image + (long)b * image_height * image_width * 3, faces_uv + (long)fn * 6, r, ts, image_height,
               image_width, wrapping, use_bilinear, tex);
}

// The transpose's entries before sorting: one lane per texel i writes its `taps` (4 bilinear, 1 nearest) entries
// e = i * taps + j as (pixel[e], weight[e]).  Entries that add nothing -- zero weight, a face outside the mask,
// CLAMP_TO_BORDER -- get pixel = H * W (past every row) and weight 0.  A stable sort by pixel then gives each pixel's
// entries in ascending (texel, tap) order.
__global__ void __launch_bounds__(256) k_uv_texture_taps(const float* __restrict__ faces_uv,
                                                         const int32_t* __restrict__ mask, long n_texels, int ts,
                                                         int image_height, int image_width, int wrapping,
                                                         int use_bilinear, int32_t* __restrict__ pixel,
                                                         float* __restrict__ weight) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n_texels) return;
    const int ts3 = ts * ts * ts;
    const int fn = (int)(i / ts3);
    const int taps = use_bilinear ? 4 : 1;
    const int none = image_height * image_width;
    TexelTaps t;
    int n = 0;
    if (!mask || mask[fn] != 0)
        n = texel_taps(faces_uv + (long)fn * 6, (int)(i - (long)fn * ts3), ts, image_height, image_width, wrapping,
                       use_bilinear, t);
#pragma unroll
    for (int j = 0; j < 4; j++) {
        if (j >= taps) break;
        const bool keep = j < n && t.w[j] != 0.0f;
        pixel[i * taps + j] = keep ? (int32_t)t.pix[j] : none;
        weight[i * taps + j] = keep ? t.w[j] : 0.0f;
    }
}

// The adjoint as a gather over the transpose (CSR, one row per pixel: row_ptr [H*W+1], entries [nnz] of (texel, weight
// bits) in ascending texel order): grad_image[b, p, k] = sum over the row of w * grad_textures[b, texel, k], in row order.
// Rows longer than long_row entries (pixel (0,0) gets one per face) go through the chunks of d3m_row_gather.h, which states
// the order: k_uv_adjoint_chunks reduces each chunk into partials [B, n_chunks, 3], and k_uv_adjoint_rows adds a long row's
// chunk sums.  No float atomics: the result is the same bits on every run.
constexpr int UV_ADJ_BLOCK = d3m::RG_BLOCK;

// one entry's term onto acc: w * g[texel], the product rounded before the sum
__device__ __forceinline__ void uv_add_entry(const int2* __restrict__ entries, const float* __restrict__ g, int e,
                                             float (&acc)[3]) {
    const int2 en = entries[e];
    const float w = __int_as_float(en.y);
    const float* gt = g + (long)en.x * 3;
#pragma unroll
    for (int k = 0; k < 3; k++) acc[k] += w * gt[k];
}

__global__ void __launch_bounds__(UV_ADJ_BLOCK) k_uv_adjoint_chunks(const int2* __restrict__ entries,
                                                                    const int2* __restrict__ chunks, int n_chunks,
                                                                    const float* __restrict__ grad_textures,
                                                                    long n_texels, float* __restrict__ partials) {
    const int c = blockIdx.x, b = blockIdx.y;
    const float* g = grad_textures + (long)b * n_texels * 3;
    float sum[3];
    d3m::rg_chunk_sum(chunks[c], sum, [&](int e, float (&acc)[3]) { uv_add_entry(entries, g, e, acc); });
    if (threadIdx.x == 0) {
        float* out = partials + ((long)b * n_chunks + c) * 3;
        out[0] = sum[0]; out[1] = sum[1]; out[2] = sum[2];
    }
}

// LPR lanes per row (a power of two up to 64, chosen from the layout's mean row length): lane `sub` of a row sums its
// entries sub, sub + LPR, ... in order, then a butterfly over the row's lanes -- the order is fixed for a given LPR.
template <int LPR>
__global__ void __launch_bounds__(256) k_uv_adjoint_rows(d3m::CsrRows transpose, const float* __restrict__ partials,
                                                         const float* __restrict__ grad_textures, long n_texels,
                                                         float* __restrict__ grad_image, int n_pixels) {
    const d3m::LongRows& longs = transpose.longs;
    const int32_t* row_ptr = transpose.offsets;
    const int2* entries = reinterpret_cast<const int2*>(transpose.items);
    const int n_chunks = longs.n_chunks;
    const long t = (long)blockIdx.x * 256 + threadIdx.x;
    const int sub = (int)(t % LPR);
    const int p = (int)min(t / LPR, (long)n_pixels);          // (lanes past the last row walk an empty row: no early exit
    const int b = blockIdx.y;                                  //  before the shuffles)
    const bool valid = p < n_pixels;
    const int start = valid ? row_ptr[p] : 0, end = valid ? row_ptr[p + 1] : 0;
    float acc[3] = {0, 0, 0};
    if (d3m::rg_is_long(longs, end - start)) {
        if (sub == 0) d3m::rg_add_chunk_sums(longs, d3m::rg_find_long(longs, p), partials + (long)b * n_chunks * 3, acc);
    } else {
        const float* g = grad_textures + (long)b * n_texels * 3;
        for (int e = start + sub; e < end; e += LPR) uv_add_entry(entries, g, e, acc);
    }
#pragma unroll
    for (int k = 0; k < 3; k++)
#pragma unroll
        for (int off = LPR / 2; off >= 1; off >>= 1) acc[k] += __shfl_xor(acc[k], off, 64);
    if (valid && sub == 0) {
        float* out = grad_image + ((long)b * n_pixels + p) * 3;
        out[0] = acc[0]; out[1] = acc[1]; out[2] = acc[2];
    }
}

// One lane per atlas pixel.  The reference's second launch (CTK:97-115) copies the finished pixel (x-1, y) onto
// the pixels just right of each tile's diagonal; (x-1, y) is never such a pixel itself and lies in the same tile,
// so evaluating this lane at x-1 gives the identical value in one pass.  Padding tiles (fn >= num_faces, where the
// reference reads out of bounds) keep zeros.
__global__ void __launch_bounds__(256) k_create_texture_image(const float* __restrict__ vertices_all,
                                                              const float* __restrict__ textures,
                                                              float* __restrict__ image, long n_pixels, int num_faces,
                                                              int tsi, int tso, int tile_width, float eps) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n_pixels) return;
    const int width = tile_width * tso;
    int x = (int)(i % width);
    const int y = (int)(i / width);
    if ((y % tso + 1) == (x % tso)) x -= 1;
    const int fn = x / tso + (y / tso) * tile_width;
    float* out = image + i * 3;
    if (fn >= num_faces) { out[0] = 0; out[1] = 0; out[2] = 0; return; }
    const float* texture = textures + (long)fn * tsi * tsi * tsi * 3;
    const float* p0 = vertices_all + (long)fn * 6;
    const float* p1 = p0 + 2;
    const float* p2 = p0 + 4;
    float face_inv[9] = {
        p1[1] - p2[1], p2[0] - p1[0], p1[0] * p2[1] - p2[0] * p1[1],
        p2[1] - p0[1], p0[0] - p2[0], p2[0] * p0[1] - p0[0] * p2[1],
        p0[1] - p1[1], p1[0] - p0[0], p0[0] * p1[1] - p1[0] * p0[1]};
    const float den = p2[0] * (p0[1] - p1[1]) + p0[0] * (p1[1] - p2[1]) + p1[0] * (p2[1] - p0[1]);
#pragma unroll
    for (int k = 0; k < 9; k++) face_inv[k] /= den;
    float weight[3], weight_sum = 0;
#pragma unroll
    for (int k = 0; k < 3; k++) {
        weight[k] = face_inv[3 * k + 0] * (float)x + face_inv[3 * k + 1] * (float)y + face_inv[3 * k + 2];
        weight_sum += weight[k];
    }
    float tif[3];
#pragma unroll
    for (int k = 0; k < 3; k++) {
        weight[k] /= (weight_sum + eps);
        float t = weight[k] * (float)(tsi - 1);
        t = fmaxf(t, 0.0f);
        t = fminf(t, (float)(tsi - 1) - eps);
        tif[k] = t;
    }
    float px[3] = {0, 0, 0};
#pragma unroll
    for (int pn = 0; pn < 8; pn++) {
        float w = 1;
        int tii[3];
#pragma unroll
        for (int k = 0; k < 3; k++) {
            const int fl = (int)tif[k];
            if (((pn >> k) & 1) == 0) { w *= 1 - (tif[k] - (float)fl); tii[k] = fl; }
            else                      { w *= tif[k] - (float)fl;       tii[k] = fl + 1; }
        }
        // tsi == 1 makes the reference index one cube past this face (weight -eps); stay inside the array
        const int isc = tii[0] * tsi * tsi + tii[1] * tsi + tii[2];
        const bool in_range = (long)fn * tsi * tsi * tsi + isc < (long)num_faces * tsi * tsi * tsi;
#pragma unroll
        for (int k = 0; k < 3; k++) px[k] += w * (in_range ? texture[isc * 3 + k] : 0.0f);
    }
    out[0] = px[0]; out[1] = px[1]; out[2] = px[2];
}
