// d3m_uv_texture.h -- per-pixel uv texture images: a texture image [H, W, C] (channels last) looked up bilinearly at the
// interpolated uv of every pixel of a coverage record (AttrMaps, d3m_fragments.h) into images [B, C, s, s], and the adjoint
// with respect to the texture image.  faces_uv [F, 3, 2], the per-corner uv of load_textures, is a constant.
//
// Wrapping is applied to the CORNERS, as load_textures defines it: corner c of face f has uv_c = wrap_uv(faces_uv[f][c])
// (d3m_textures.h; REPEAT, MIRRORED_REPEAT or CLAMP_TO_EDGE -- CLAMP_TO_BORDER is refused, nearest lookup is not offered); a
// fill_back copy (fn >= F) reads corners 2 - c, as it reads vertices.  Internal pixel p of view b with owner fn >= 0:
//   u_c   = va_weights (d3m_fragments.h): weight_map[b,p,c] * (depth_map[b,p] / faces[b,fn,c,2]);
//   pu    = (u_0 uv_0.x + u_1 uv_1.x) + u_2 uv_2.x, pv likewise with .y;
//   pos_x = clamp(pu (W - 1), 0, W - 1), pos_y = clamp(pv (H - 1), 0, H - 1) -- the u_c sum to 1 and the wrapped corners lie
//           in [0, 1], so the clamp only absorbs rounding (and sends a NaN to 0: every tap is inside the image);
//   from pos on, bilinear_taps (d3m_textures.h), the taps and weights of texel_taps: xi = (int)pos_x, yi = (int)pos_y,
//           y1 = min((int)(pos_y + 1), H - 1), x1 = min(xi + 1, W - 1), order p00, p10, p01, p11;
//   value[k] = sum_j image[tap_j][k] * w_j, added in that order from 0;
// an uncovered pixel takes background[k].  Value and tap weights are continuous in pos (except where the f32 sum pos_y + 1
// rounds up to the next integer: the last f32 below 1, 3, 7, ... -- LTK's own rule, kept).  The output image is what
// k_vertex_attribute_images makes of such a map: rows reversed and, with anti-aliasing, ((p00 + p01) + p10) + p11 in OUTPUT
// orientation, times 1/4.  alpha is the coverage treated the same way: the bits of k_vertex_attribute_images' alpha.
//
// THE ADJOINT is a scatter whose destinations change with every coverage, so no transpose can be built once.  It is
// independent of order BY CONSTRUCTION -- a fixed-point sum in 64-bit integers -- and uses no float atomics:
//   term     t = w_j * (scale * g[b, k, out(p)]) in f32, scale = 1 or 1/4, for internal pixel p, tap j, channel k;
//   gmax     max |scale * g| over the call, taken on the bits of |x| as unsigned (NaN > Inf > finite): per-workgroup maxima
//            with plain stores (k_uv_texture_images_clear_max), combined by every workgroup that reads them (a max does
//            not depend on order);
//   quantum  E = ilogb(gmax) + 1, frac = 62 - ceil(log2(B S S)) (the host passes it), q = 2^(E - frac);
//   add      __double2ll_rn((double)t * 2^(frac - E)) with a 64-bit INTEGER atomic add into one int64 accumulator per element
//            of grad_image (a shared image: the views add into the same accumulators); k_uv_texture_images_clear_max clears
//            the accumulators first -- nothing is assumed of the caller's scratch;
//   convert  grad_image = (float)((double)acc * 2^(E - frac)).
// Integer sums are associative, so neither arrival order nor launch shape can change a bit.  |t| <= gmax < 2^E (every
// w_j <= 1) and a pixel's four weights sum to 1, so |sum| <= B S^2 2^frac <= 2^62 plus at most 2 B S^2 of rounding: no
// overflow; B S^2 > 2^32 (frac < 30) is refused.  gmax == 0: the scatter is skipped, every element is an exact +0, nothing is
// divided by gmax.  gmax not finite (an Inf or a NaN in g): the scatter is skipped and every element is NaN.  A texel that no
// sample reaches (and a sum that cancels) is +0.  Everything reads gmax from device memory: nothing goes back to the host.
// Launches: 1 forward; 3 backward (clear + block maxima, scatter, convert).
#pragma once
#include "d3m_fragments.h"
#include "d3m_textures.h"

namespace d3m {

constexpr int UVT_CHUNK = VA_CHUNK;      // channels a lane of the forward keeps in registers at a time
constexpr int UVT_MAX_CHANNELS = 64;
constexpr int UVT_MAX_SIZE = 32768;      // H, W: W - 1 and every tap index are exact in f32, H W fits an int
constexpr int UVT_MAX_BLOCKS = 1024;     // workgroups of k_uv_texture_images_clear_max = block maxima in the scratch
constexpr int UVT_SCATTER_BLOCKS = 2048; // the scatter's fixed grid

struct UvTexture {
    const float* faces_uv;               // [Ft,3,2]
    int H, W, C, image_batch, wrapping;
};

struct UvtTaps {
    int pix[4];                          // y * W + x
    float w[4];
};

struct UvtCorners {
    float u[3], cx[3], cy[3];            // va_weights; the owner's wrapped corner uv (a fill_back copy: corners 2 - c)
};

// the level-0 position of internal pixel q (index into the batch's maps) owned by fn, whose corner depths are z[0..2]: the
// one statement of pos for this node and for the mip-mapped one (d3m_uv_texture_mip.h), which also reads the corners
__device__ __forceinline__ void uvt_pixel_position(const AttrMaps& m, const UvTexture& tx, size_t q, int fn, const float* z,
                                                   UvtCorners& k, float& pos_x, float& pos_y) {
    const bool back = fn >= m.Ft;
    const float* uvf = tx.faces_uv + (size_t)(back ? fn - m.Ft : fn) * 6;
    va_weights(m, q, z, k.u);
#pragma unroll
    for (int c = 0; c < 3; c++) {
        const int cc = back ? 2 - c : c;
        k.cx[c] = wrap_uv(uvf[2 * cc], tx.wrapping);
        k.cy[c] = wrap_uv(uvf[2 * cc + 1], tx.wrapping);
    }
    const float pu = (k.u[0] * k.cx[0] + k.u[1] * k.cx[1]) + k.u[2] * k.cx[2];
    const float pv = (k.u[0] * k.cy[0] + k.u[1] * k.cy[1]) + k.u[2] * k.cy[2];
    const float x_max = (float)(tx.W - 1), y_max = (float)(tx.H - 1);
    pos_x = fminf(fmaxf(pu * x_max, 0.0f), x_max);
    pos_y = fminf(fmaxf(pv * y_max, 0.0f), y_max);
}

// the taps of internal pixel q of view b, owned by fn
__device__ __forceinline__ void uvt_pixel_taps(const AttrMaps& m, const UvTexture& tx, int b, size_t q, int fn, UvtTaps& t) {
    float z[3];
    fr_corner_depths(m, b, fn, z);
    UvtCorners k;
    float pos_x, pos_y;
    uvt_pixel_position(m, tx, q, fn, z, k, pos_x, pos_y);
    TexelTaps tt;
    bilinear_taps(pos_x, pos_y, tx.H, tx.W, tt);
#pragma unroll
    for (int j = 0; j < 4; j++) {
        t.pix[j] = (int)tt.pix[j];
        t.w[j] = tt.w[j];
    }
}

// ---- forward: fr_output_pixel_walk (d3m_fragments.h) over the four taps of every internal pixel ----------------------------
__global__ void __launch_bounds__(256) k_uv_texture_images(AttrMaps m, UvTexture tx, const float* __restrict__ image,
                                                          const float* __restrict__ background, float* __restrict__ images,
                                                          float* __restrict__ alpha) {
    const int C = tx.C;
    const float* img = image + (size_t)(tx.image_batch > 1 ? (int)blockIdx.y : 0) * tx.H * tx.W * C;
    UvtTaps taps[4];
    fr_output_pixel_walk(
        m, C, background, images, alpha, [&](int j, int b, size_t q, int fn) { uvt_pixel_taps(m, tx, b, q, fn, taps[j]); },
        [&](int j, int k) {
            float v = 0.0f;
#pragma unroll
            for (int a = 0; a < 4; a++) v += img[(size_t)taps[j].pix[a] * C + k] * taps[j].w[a];
            return v;
        });
}

// ---- adjoint ------------------------------------------------------------------------------------------------------------
// max over the workgroup's 256 lanes, returned to every lane (one call per kernel)
__device__ __forceinline__ unsigned uvt_block_max(unsigned v) {
    __shared__ unsigned s_max[4];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = max(v, (unsigned)__shfl_xor((int)v, o));
    if ((threadIdx.x & 63) == 0) s_max[threadIdx.x >> 6] = v;
    __syncthreads();
    return max(max(s_max[0], s_max[1]), max(s_max[2], s_max[3]));
}

// gmax's bits from the block maxima: every workgroup of the scatter and of the convert combines them itself
__device__ __forceinline__ unsigned uvt_gmax_bits(const unsigned* __restrict__ block_max, int n_max) {
    unsigned v = 0;
    for (int i = threadIdx.x; i < n_max; i += 256) v = max(v, block_max[i]);
    return uvt_block_max(v);
}

enum { UVT_ZERO = 0, UVT_FINITE = 1, UVT_NOT_FINITE = 2 };
struct UvtQuantum {
    int state;
    double up, down;                     // 2^(frac - E), 2^(E - frac)
};

__device__ __forceinline__ UvtQuantum uvt_quantum(unsigned gmax_bits, int frac) {
    UvtQuantum qn{UVT_FINITE, 0.0, 0.0};
    if (gmax_bits == 0) qn.state = UVT_ZERO;
    else if (gmax_bits >= 0x7F800000u) qn.state = UVT_NOT_FINITE;
    else {
        const int e = (int)(gmax_bits >> 23);
        const int E = (e ? e - 127 : (31 - __clz((int)gmax_bits)) - 149) + 1;       // ilogb(gmax) + 1, subnormals included
        qn.up = ldexp(1.0, frac - E);
        qn.down = ldexp(1.0, E - frac);
    }
    return qn;
}

// 1. a fixed grid clears the n_acc accumulators and leaves each workgroup's max of the bits of |scale * g| in block_max
__global__ void __launch_bounds__(256) k_uv_texture_images_clear_max(const float* __restrict__ grad_images, long n_g, float scale,
                                                                    unsigned long long* __restrict__ acc, long n_acc,
                                                                    unsigned* __restrict__ block_max) {
    const long first = (long)blockIdx.x * 256 + threadIdx.x, stride = (long)gridDim.x * 256;
    for (long i = first; i < n_acc; i += stride) acc[i] = 0ull;
    unsigned v = 0;
    for (long i = first; i < n_g; i += stride) v = max(v, __float_as_uint(scale * grad_images[i]) & 0x7FFFFFFFu);
    v = uvt_block_max(v);
    if (threadIdx.x == 0) block_max[blockIdx.x] = v;
}

// 2. one lane per internal pixel of a fixed grid striding over B S S quantises and atomically adds the TAPS taps of every
// owned pixel: term = w_j * (scale * g), a tap of weight 0 adds nothing and is skipped.  The channel loop is innermost, so a
// lane's adds to one tap are C * 8 contiguous bytes.  taps(b, p, fn, pix, w): the pixel's tap texels (within one image's
// per_image / C accumulator texels) and weights; acc holds per_image accumulators an image.
template <int TAPS, class Taps>
__device__ __forceinline__ void uvt_scatter_taps(const AttrMaps& m, int C, int image_batch, size_t per_image,
                                                 const float* __restrict__ grad_images, const unsigned* __restrict__ block_max,
                                                 int n_max, int frac, unsigned long long* __restrict__ acc, Taps taps) {
    const UvtQuantum qn = uvt_quantum(uvt_gmax_bits(block_max, n_max), frac);
    if (qn.state != UVT_FINITE) return;
    const int s = fr_output_size(m);
    const long n = (long)m.B * m.S * m.S;
    const float scale = m.aa ? 0.25f : 1.0f;
    for (long p = (long)blockIdx.x * 256 + threadIdx.x; p < n; p += (long)gridDim.x * 256) {
        int b, x, y, fn, xo, yo;
        fr_pixel(m, p, b, x, y, fn);
        if (fn < 0) continue;
        int pix[TAPS];
        float w[TAPS];
        taps(b, (size_t)p, fn, pix, w);
        fr_output_pixel(m, x, y, xo, yo);
        const float* g = grad_images + ((size_t)b * C * s + yo) * s + xo;
        unsigned long long* dst = acc + (size_t)(image_batch > 1 ? b : 0) * per_image;
#pragma unroll
        for (int j = 0; j < TAPS; j++) {
            if (w[j] == 0.0f) continue;
            unsigned long long* texel = dst + (size_t)pix[j] * C;
            for (int k = 0; k < C; k++) {
                const float term = w[j] * (scale * g[(size_t)k * s * s]);
                const long long fixed = __double2ll_rn((double)term * qn.up);
                __hip_atomic_fetch_add(texel + k, (unsigned long long)fixed, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
        }
    }
}

__global__ void __launch_bounds__(256) k_uv_texture_images_scatter(AttrMaps m, UvTexture tx, const float* __restrict__ grad_images,
                                                                  const unsigned* __restrict__ block_max, int n_max, int frac,
                                                                  unsigned long long* __restrict__ acc) {
    uvt_scatter_taps<4>(m, tx.C, tx.image_batch, (size_t)tx.H * tx.W * tx.C, grad_images, block_max, n_max, frac, acc,
                        [&](int b, size_t q, int fn, int* pix, float* w) {
                            UvtTaps t;
                            uvt_pixel_taps(m, tx, b, q, fn, t);
#pragma unroll
                            for (int j = 0; j < 4; j++) {
                                pix[j] = t.pix[j];
                                w[j] = t.w[j];
                            }
                        });
}

// 3. one lane per element of grad_image (a fixed grid striding over them); every element is written
__global__ void __launch_bounds__(256) k_uv_texture_images_convert(const long long* __restrict__ acc, long n_acc,
                                                                  const unsigned* __restrict__ block_max, int n_max, int frac,
                                                                  float* __restrict__ grad_image) {
    const UvtQuantum qn = uvt_quantum(uvt_gmax_bits(block_max, n_max), frac);
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n_acc; i += (long)gridDim.x * 256) {
        float v = 0.0f;
        if (qn.state == UVT_FINITE) v = (float)((double)acc[i] * qn.down);
        else if (qn.state == UVT_NOT_FINITE) v = __uint_as_float(0x7FC00000u);
        grad_image[i] = v;
    }
}

}  // namespace d3m
