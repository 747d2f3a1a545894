// d3m_uv_bake.h -- view images baked into a uv texture: the inverse of the per-pixel uv texture images (d3m_uv_texture.h).  Two
// coverage records (AttrMaps, d3m_fragments.h) meet here: the LAYOUT record `uv` -- B = 1, S = T, the faces_uv layout
// rasterised with z = 1 by uv_layout_fragments, so that weight_map holds a texel's barycentrics b_c in its owner -- shared by the
// views and never expanded, and the VIEW record `vw` of B views with its z-buffer.  images [B, C, H, W] in output orientation
// (row 0 = top, any H, W) -> texture [B, T, T, C] (channels last: what sample_uv_texture takes) and mask [B, T, T].
//
// Texel p (index into the layout's maps; internal row j is texture row j) of view b, with layout owner f >= 0, underlying
// mesh triangle t = f mod Ft (Ft the number of triangles of BOTH records):
//   corners  (x_c, y_c, z_c) = screen_vertices[b, tri[t][c]], tri the view record's; a fill_back copy (f >= Ft) reads
//            tri[t][2 - c], as it reads its uv corners;
//   point    perspective:  t_c = b_c z_c, Z = (t_0 + t_1) + t_2, x = ((t_0 x_0 + t_1 x_1) + t_2 x_2) / Z, y likewise -- the
//            screen-space point that the rasteriser's perspective-correct weights give the barycentrics b_c;
//            orthographic: x = (b_0 x_0 + b_1 x_1) + b_2 x_2, y likewise, Z as above;
//   visible  (a CONSTANT of the graph)  gx = (x S + S) / 2, gy = (y S + S) / 2, S the view record's raster size; invisible
//            unless 0 <= gx < S and 0 <= gy < S (a NaN is outside); (px, py) = ((int)gx, (int)gy), the internal pixel whose
//            area holds the point, o its owner: invisible when uncovered; else visible iff o mod Ft == t (either copy) or
//            Z <= depth_map[b,py,px] + depth_tolerance.  The triangle's orientation in the view is not tested;
//   lookup   col = clamp((x W + W - 1) / 2, 0, W - 1), row = clamp((H - 1) - (y H + H - 1) / 2, 0, H - 1) (a NaN goes to
//            0: every tap is inside the image); xi = (int)col, fx = col - xi, x1 = min(xi + 1, W - 1), yi, fy, y1 likewise;
//            taps in the order t00 = (yi, xi), t01 = (yi, x1), t10 = (y1, xi), t11 = (y1, x1) with weights (1 - fx)(1 - fy),
//            fx (1 - fy), (1 - fx) fy, fx fy: value and weights are continuous in (col, row);
//   value    texture[b,p,k] = sum_j images[b,k,tap_j] * w_j, added in that order from 0, for a visible texel, else
//            background[k] (0 without one); mask[b,p] = 1 or 0.  A texel that no uv triangle covers: background, mask 0.
// Every element of texture and mask is written.  One launch: a lane per texel, blockIdx.y = the view, channels in chunks of
// VA_CHUNK.
//
// THE ADJOINT IN THE IMAGES is a scatter whose destinations change with the geometry: the fixed-point sum of d3m_uv_texture.h
// (its clear + block maxima and its convert kernels, scale 1): term = w_j * g[b,p,k] for every visible texel, quantised to
// q = 2^(E - frac), E = ilogb(max |g|) + 1, and added with a 64-bit INTEGER atomic into one int64 accumulator per element of
// grad_images.  View b's image receives only from view b's T^2 texels, whose four weights sum to 1: frac = 62 -
// ceil(log2(T^2)) cannot overflow.  gmax == 0: every element an exact +0; gmax not finite: every element NaN.  Three launches.
//
// THE ADJOINT IN THE SCREEN VERTICES.  Visibility and the choice of taps are constants.  Per visible texel, g_k = g[b,p,k]:
//   Dcol = sum over k ascending of g_k * ((1 - fy)(t01 - t00) + fy (t11 - t10)),  0 unless 0 < col < W - 1;
//   Drow = sum over k ascending of g_k * ((1 - fx)(t10 - t00) + fx (t11 - t01)),  0 unless 0 < row < H - 1;
//   Gx = dL/dx = Dcol W / 2,  Gy = dL/dy = -Drow H / 2;
//   perspective:  dL/dx_c = Gx b_c z_c / Z,  dL/dy_c = Gy b_c z_c / Z,  dL/dz_c = (b_c / Z)(Gx (x_c - x) + Gy (y_c - y));
//   orthographic: dL/dx_c = Gx b_c,  dL/dy_c = Gy b_c,  dL/dz_c = +0.
// Stage 1: nine accumulators (corner-major, acc[3 c + j]) per (view, layout face), summed over the texels the face owns in
// THE ORDER of d3m_fragments.h (fr_face_sums / fr_large_face_sums over the LAYOUT record, blockIdx.y = the view), stored at
// Gv[(view F' + f) 9 ...].  Stage 2: the rows / chunks gather of d3m_attributes.h over the MESH's vertex adjacency with C = 3,
// a result per view: a layout face and its fill_back copy fold onto the one mesh triangle (the copy's corner 2 - c is the
// triangle's corner c, which is how the gather reads a copy).  The gather reads the layout's visibility flags once per view
// (k_uv_bake_view_flags copies them: B rows of F').  No float atomics, nothing cleared, the same bits on every run.
// Launches: forward 1; images 3; vertices 4 (the flags, the two face-sum kernels, the rows) and the chunks on a mesh with long rows.
#pragma once
#include "d3m_attributes.h"
#include "d3m_uv_texture.h"

namespace d3m {

// what the kernels read of the view record (the kernels take two records: the arguments are kept few)
struct UbView {
    const int32_t* face_index_map;       // [B,S,S]
    const float* depth_map;              // [B,S,S]
    const int32_t* tri;                  // [Ft,3]
    int S, Ft, Fp;
};

struct UvBake {
    const float* screen_vertices;        // [B,V,3]
    const float* images;                 // [B,C,H,W]
    int V, C, H, W, perspective;
    float depth_tolerance;
};

// a texel's owner in view b: its barycentrics, the owner's corners and the surface point
struct UbPoint {
    float bw[3], cx[3], cy[3], cz[3];
    float x, y, Z;
};

struct UbTaps {
    int pix[4];                          // y * W + x of t00, t01, t10, t11
    float w[4];
    float fx, fy;
    bool inner_x, inner_y;               // 0 < col < W - 1, 0 < row < H - 1
};

// the corners of layout owner f in view b; false for a triangle index outside the vertices (nothing is read through it)
__device__ __forceinline__ bool ub_corners(const UbView& vw, const UvBake& bk, int b, int f, UbPoint& p) {
    const bool back = f >= vw.Ft;
    const int32_t* t = vw.tri + (size_t)(back ? f - vw.Ft : f) * 3;
    const float* sv = bk.screen_vertices + (size_t)b * bk.V * 3;
    const int t0 = t[0], t1 = t[1], t2 = t[2];
    const int v[3] = {back ? t2 : t0, t1, back ? t0 : t2};
    if ((unsigned)t0 >= (unsigned)bk.V || (unsigned)t1 >= (unsigned)bk.V || (unsigned)t2 >= (unsigned)bk.V) return false;
#pragma unroll
    for (int c = 0; c < 3; c++) {
        p.cx[c] = sv[3 * (size_t)v[c]];
        p.cy[c] = sv[3 * (size_t)v[c] + 1];
        p.cz[c] = sv[3 * (size_t)v[c] + 2];
    }
    return true;
}

// the surface point of layout pixel q, whose corners are already in p
__device__ __forceinline__ void ub_point(const AttrMaps& uv, const UvBake& bk, size_t q, UbPoint& p) {
#pragma unroll
    for (int c = 0; c < 3; c++) p.bw[c] = uv.weight_map[3 * q + c];
    const float t0 = p.bw[0] * p.cz[0], t1 = p.bw[1] * p.cz[1], t2 = p.bw[2] * p.cz[2];
    p.Z = (t0 + t1) + t2;
    if (bk.perspective) {
        p.x = ((t0 * p.cx[0] + t1 * p.cx[1]) + t2 * p.cx[2]) / p.Z;
        p.y = ((t0 * p.cy[0] + t1 * p.cy[1]) + t2 * p.cy[2]) / p.Z;
    } else {
        p.x = (p.bw[0] * p.cx[0] + p.bw[1] * p.cx[1]) + p.bw[2] * p.cx[2];
        p.y = (p.bw[0] * p.cy[0] + p.bw[1] * p.cy[1]) + p.bw[2] * p.cy[2];
    }
}

// the z-buffer test of the point of layout owner f in view b
__device__ __forceinline__ bool ub_visible(const UbView& vw, const UvBake& bk, int b, int f, const UbPoint& p) {
    const float S = (float)vw.S;
    const float gx = (p.x * S + S) * 0.5f, gy = (p.y * S + S) * 0.5f;
    if (!(gx >= 0.0f && gx < S && gy >= 0.0f && gy < S)) return false;
    const size_t q = ((size_t)b * vw.S + (int)gy) * vw.S + (int)gx;
    const int o = vw.face_index_map[q];
    if ((unsigned)o >= (unsigned)vw.Fp) return false;
    const int t = f >= vw.Ft ? f - vw.Ft : f;
    if ((o >= vw.Ft ? o - vw.Ft : o) == t) return true;
    return p.Z <= vw.depth_map[q] + bk.depth_tolerance;
}

__device__ __forceinline__ void ub_taps(const UvBake& bk, const UbPoint& p, UbTaps& t) {
    const float W = (float)bk.W, H = (float)bk.H, x_max = (float)(bk.W - 1), y_max = (float)(bk.H - 1);
    const float col = fminf(fmaxf((p.x * W + x_max) * 0.5f, 0.0f), x_max);
    const float row = fminf(fmaxf(y_max - (p.y * H + y_max) * 0.5f, 0.0f), y_max);
    const int xi = (int)col, yi = (int)row;
    const int x1 = min(xi + 1, bk.W - 1), y1 = min(yi + 1, bk.H - 1);
    t.fx = col - (float)xi;
    t.fy = row - (float)yi;
    const float wx0 = 1.0f - t.fx, wy0 = 1.0f - t.fy;
    t.pix[0] = yi * bk.W + xi; t.w[0] = wx0 * wy0;
    t.pix[1] = yi * bk.W + x1; t.w[1] = t.fx * wy0;
    t.pix[2] = y1 * bk.W + xi; t.w[2] = wx0 * t.fy;
    t.pix[3] = y1 * bk.W + x1; t.w[3] = t.fx * t.fy;
    t.inner_x = col > 0.0f && col < x_max;
    t.inner_y = row > 0.0f && row < y_max;
}

// texel q of the layout in view b: false when uncovered or invisible, else its point and taps
__device__ __forceinline__ bool ub_texel(const AttrMaps& uv, const UbView& vw, const UvBake& bk, int b, size_t q, UbPoint& p,
                                         UbTaps& t) {
    const int f = uv.face_index_map[q];
    if ((unsigned)f >= (unsigned)uv.Fp) return false;
    if (!ub_corners(vw, bk, b, f, p)) return false;
    ub_point(uv, bk, q, p);
    if (!ub_visible(vw, bk, b, f, p)) return false;
    ub_taps(bk, p, t);
    return true;
}

// ---- forward: a lane per texel, blockIdx.y = the view -------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_uv_bake_texture(AttrMaps uv, UbView vw, UvBake bk, const float* __restrict__ background,
                                                        float* __restrict__ texture, float* __restrict__ mask) {
    const long T2 = (long)uv.S * uv.S;
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    const int b = blockIdx.y, C = bk.C;
    if (i >= T2) return;
    UbPoint p;
    UbTaps t;
    const bool visible = ub_texel(uv, vw, bk, b, (size_t)i, p, t);
    const size_t plane = (size_t)bk.H * bk.W;
    const float* img = bk.images + (size_t)b * C * plane;
    float* out = texture + ((size_t)b * T2 + i) * C;
    for (int k0 = 0; k0 < C; k0 += VA_CHUNK) {
        float v[VA_CHUNK];
#pragma unroll
        for (int kk = 0; kk < VA_CHUNK; kk++) {
            const int k = k0 + kk;
            v[kk] = 0.0f;
            if (k >= C) continue;
            if (visible) {
                const float* ch = img + (size_t)k * plane;
#pragma unroll
                for (int j = 0; j < 4; j++) v[kk] += ch[t.pix[j]] * t.w[j];
            } else {
                v[kk] = background ? background[k] : 0.0f;
            }
        }
#pragma unroll
        for (int kk = 0; kk < VA_CHUNK; kk++)
            if (k0 + kk < C) out[k0 + kk] = v[kk];
    }
    mask[(size_t)b * T2 + i] = visible ? 1.0f : 0.0f;
}

// ---- the adjoint in the images: the scatter between d3m_uv_texture.h's clear + maxima and its convert ----------------------------
// a fixed grid strides over a view's texels, blockIdx.y = the view; acc [B,C,H,W] int64; a tap of weight 0 adds nothing
__global__ void __launch_bounds__(256) k_uv_bake_images_scatter(AttrMaps uv, UbView vw, UvBake bk,
                                                               const float* __restrict__ grad_texture,
                                                               const unsigned* __restrict__ block_max, int n_max, int frac,
                                                               unsigned long long* __restrict__ acc) {
    const UvtQuantum qn = uvt_quantum(uvt_gmax_bits(block_max, n_max), frac);
    if (qn.state != UVT_FINITE) return;
    const long T2 = (long)uv.S * uv.S;
    const int b = blockIdx.y, C = bk.C;
    const size_t plane = (size_t)bk.H * bk.W;
    unsigned long long* dst = acc + (size_t)b * C * plane;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < T2; i += (long)gridDim.x * 256) {
        UbPoint p;
        UbTaps t;
        if (!ub_texel(uv, vw, bk, b, (size_t)i, p, t)) continue;
        const float* g = grad_texture + ((size_t)b * T2 + i) * C;
        for (int k = 0; k < C; k++) {
            const float gk = g[k];
#pragma unroll
            for (int j = 0; j < 4; j++) {
                if (t.w[j] == 0.0f) continue;
                const long long fixed = __double2ll_rn((double)(t.w[j] * gk) * qn.up);
                __hip_atomic_fetch_add(dst + (size_t)k * plane + t.pix[j], (unsigned long long)fixed, __ATOMIC_RELAXED,
                                       __HIP_MEMORY_SCOPE_AGENT);
            }
        }
    }
}

// ---- the adjoint in the screen vertices, stage 1: fr_face_sums / fr_large_face_sums over the layout record ------------------------
// The walks hand a policy the layout face's nine floats, not its index: a texel reads its owner from the map, and the owner's
// corners through it (every texel of one walk has the same owner: the loads hit the cache).
struct UbFaceSums {
    const AttrMaps& uv;
    const UbView& vw;
    const UvBake& bk;
    const float* grad_texture;
    float* Gv;
    int view;
    __device__ __forceinline__ void setup(const float*, int) const {}
    __device__ __forceinline__ void add(int, int, size_t q, float* acc) const {
        const int f = uv.face_index_map[q];
        UbPoint p;
        if (!ub_corners(vw, bk, view, f, p)) return;
        ub_point(uv, bk, q, p);
        if (!ub_visible(vw, bk, view, f, p)) return;
        UbTaps t;
        ub_taps(bk, p, t);
        const int C = bk.C;
        const size_t plane = (size_t)bk.H * bk.W;
        const float* img = bk.images + (size_t)view * C * plane;
        const float* g = grad_texture + ((size_t)view * uv.S * uv.S + q) * C;
        float dcol = 0.0f, drow = 0.0f;
        for (int k = 0; k < C; k++) {
            const float* ch = img + (size_t)k * plane;
            const float a00 = ch[t.pix[0]], a01 = ch[t.pix[1]], a10 = ch[t.pix[2]], a11 = ch[t.pix[3]];
            const float gk = g[k];
            dcol += gk * ((1.0f - t.fy) * (a01 - a00) + t.fy * (a11 - a10));
            drow += gk * ((1.0f - t.fx) * (a10 - a00) + t.fx * (a11 - a01));
        }
        if (!t.inner_x) dcol = 0.0f;
        if (!t.inner_y) drow = 0.0f;
        const float gx = dcol * (0.5f * (float)bk.W), gy = -(drow * (0.5f * (float)bk.H));
        // (the orthographic z term is an exact +0: the sums stay +0)
        const bool persp = bk.perspective != 0;
        const float s0 = persp ? p.bw[0] * p.cz[0] / p.Z : p.bw[0];
        const float s1 = persp ? p.bw[1] * p.cz[1] / p.Z : p.bw[1];
        const float s2 = persp ? p.bw[2] * p.cz[2] / p.Z : p.bw[2];
        const float z0 = persp ? (p.bw[0] / p.Z) * (gx * (p.cx[0] - p.x) + gy * (p.cy[0] - p.y)) : 0.0f;
        const float z1 = persp ? (p.bw[1] / p.Z) * (gx * (p.cx[1] - p.x) + gy * (p.cy[1] - p.y)) : 0.0f;
        const float z2 = persp ? (p.bw[2] / p.Z) * (gx * (p.cx[2] - p.x) + gy * (p.cy[2] - p.y)) : 0.0f;
        acc[0] += gx * s0; acc[1] += gy * s0; acc[2] += z0;
        acc[3] += gx * s1; acc[4] += gy * s1; acc[5] += z1;
        acc[6] += gx * s2; acc[7] += gy * s2; acc[8] += z2;
    }
    __device__ __forceinline__ void store(size_t gi, const float* acc) const {
        float* out = Gv + ((size_t)view * uv.Fp + gi) * 9;
#pragma unroll
        for (int k = 0; k < 9; k++) out[k] = acc[k];
    }
};

__global__ void __launch_bounds__(256) k_uv_bake_face_sums(AttrMaps uv, UbView vw, UvBake bk,
                                                          const float* __restrict__ grad_texture, const int* __restrict__ list,
                                                          const int* __restrict__ n_list, float* __restrict__ Gv) {
    UbFaceSums policy{uv, vw, bk, grad_texture, Gv, (int)blockIdx.y};
    fr_face_sums<9>(uv, list, n_list, policy);
}

__global__ void __launch_bounds__(RG_BLOCK) k_uv_bake_large_face_sums(AttrMaps uv, UbView vw, UvBake bk,
                                                                     const float* __restrict__ grad_texture,
                                                                     const int* __restrict__ list,
                                                                     const int* __restrict__ n_list, float* __restrict__ Gv) {
    UbFaceSums policy{uv, vw, bk, grad_texture, Gv, (int)blockIdx.y};
    fr_large_face_sums<9>(uv, list, n_list, policy);
}

// the layout's visibility flags [F'] once per view [B,F']: what stage 2 reads beside Gv
__global__ void __launch_bounds__(256) k_uv_bake_view_flags(const int* __restrict__ flags, int Fp, int* __restrict__ view_flags) {
    const int f = blockIdx.x * 256 + threadIdx.x;
    if (f < Fp) view_flags[(size_t)blockIdx.y * Fp + f] = flags[f];
}

}  // namespace d3m
