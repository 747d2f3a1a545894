// d3m_uv_fill.h -- fuse baked view textures and fill the texels no view saw by push-pull: the step between bake_uv_texture
// (d3m_uv_bake.h) and the mip-mapped lookup (d3m_uv_texture_mip.h).  textures [B, H, W, C] and weights [B, H, W] give one
// texture [H, W, C] and valid [H, W]; without the fill the bilinear taps at chart borders and every level of the box pyramid
// average the background into the picture.  Differentiable in the textures; the weights and the set of valid texels are
// constants.  Every value below is defined by a recursion in a fixed order, so the bits do not depend on the launches.
//
// FUSION.  View b counts at texel t iff w_b[t] > 0 (a NaN and a negative weight are "not > 0": absent).  t is valid iff some
// view counts.  v0[t] = (sum_b w_b x_b) / (sum_b w_b) over the counting views in ascending b, in f32, both sums starting at the
// first counting view's term (no 0 is added in front): B = 1, w = 1 gives x bit for bit.  Without the fill the output is v0 on
// valid texels and the background elsewhere (one launch, no scratch).
//
// PULL.  Level 0 is (H, W); level l + 1 has (h + 1) >> 1 rows and (w + 1) >> 1 columns, up to the 1 x 1 level L <= 15.  s_0 = v0
// on valid texels and 0 elsewhere, n_0 = 1 / 0 (an integer);
//   s_{l+1}(y, x) = ((s_l(2y, 2x) + s_l(2y, 2x + 1)) + s_l(2y + 1, 2x)) + s_l(2y + 1, 2x + 1), n_{l+1} the same sum of n_l;
// a child outside the level contributes 0.  s_l / n_l is the mean of the valid level-0 texels under a level-l texel.
//
// PUSH.  f_L = n_L > 0 ? s_L / n_L : background.  For l = L - 1 .. 0: f_l(t) = n_l(t) > 0 ? s_l(t) / n_l(t) : up_l(t), up_l the
// bilinear value of f_{l+1} at the texel's centre.  Per axis, N2 the coarse size (uf_tap):
//   p = clamp(0.5 i - 0.25, 0, N2 - 1), i0 = min((int)p, max(N2 - 2, 0)), i1 = min(i0 + 1, N2 - 1), t = p - i0  (all exact),
//   up = (1 - ty) ((1 - tx) c00 + tx c01) + ty ((1 - tx) c10 + tx c11).
// The output is f_0: v0 bit for bit on a valid texel (n_0 = 1), the background everywhere when no texel is valid.
//
// THE ADJOINT.  Every sum is a gather in a fixed order; no atomics; the same bits on every run.
//   push adjoint, fine to coarse: G_0 = g.  G_{l+1}(j) = sum of weight(i, j) G_l(i) over the level-l texels i with n_l(i) = 0
//            whose taps include j, weight(i, j) = wy wx and per axis w = (i0 == j ? 1 - t : 0) + (i1 == j ? t : 0), in ascending
//            (row, column) order starting from +0.  The candidates are i in [2j - 2, 2j + 3] per axis, clipped to the level
//            (the clamped taps at the borders reach that far); membership is decided by uf_tap, and a term whose weight is
//            exactly 0 is skipped.  g_val_l(t) = n_l(t) > 0 ? G_l(t) : 0.
//   pull adjoint, coarse to fine: gs_0(t) of a valid texel = ((g_val_L / n_L + g_val_{L-1} / n_{L-1}) + ...) + g_val_0 / 1 over
//            its ancestors (all of them have n > 0), in that order starting from the first term.
//   fusion:  g_x_b[t] = (w_b / sum w) gs_0(t) where view b counts at t, exactly +0 elsewhere; sum w as in the forward.
// A texel filled from the background passes nothing on.  g = 0 gives +0 everywhere.  A non-finite g at a valid texel reaches
// that texel's views only; at an invalid texel it reaches, as inf or NaN, the coarse texels of its non-zero taps, upwards until
// a level where they are valid, and every view of every valid level-0 texel under those; elements not under them stay finite.
//
// LAUNCHES.  Forward 3 for every size (k_uv_fill_fuse_tile, k_uv_fill_top, k_uv_fill_push_tile), 1 without the fill.  Backward:
// k_uv_fill_adjoint_tile once per three levels while a level is larger than 32 x 32 and once more for all levels above, then
// k_uv_fill_adjoint_views: 2 up to 32 x 32, 3 up to 256 x 256, 4 up to 2048 x 2048, 6 at the largest size; 1 without the fill.
// Independent of B and C.  No memset, no waits, one stream; the scratch is the caller's (d3m_uv_fill_scratch_bytes).
#pragma once
#include "d3m_uv_texture_mip.h"

namespace d3m {

constexpr int UF_MAX_LEVEL = 15;
constexpr int UF_TOP_BLOCK = 1024;
constexpr int UF_ADJ_STEPS = 3;                           // levels one k_uv_fill_adjoint_tile launch climbs over several tiles
constexpr int UF_PUSH_WINDOW = (UVT_TILE / 2 + 2) * (UVT_TILE / 2 + 2);          // level 1 of a tile with its halo of one
constexpr int UF_ADJ_WINDOW_A = 28 * 28;                  // step 1 of 3: 16 + 2 * 6 texels a side
constexpr int UF_ADJ_WINDOW_B = 12 * 12;                  // step 2 of 3: 8 + 2 * 2

struct UvFill {
    int H, W, C, L;
    long offset[UF_MAX_LEVEL + 2];       // of level l's first texel in the pyramids (levels 1..L; offset[1] = 0, offset[L + 1] = all)
};

__host__ __device__ inline int uf_size(int n, int l) { return ((n - 1) >> l) + 1; }

struct UfTap {
    int i0, i1;
    float t;
};

__device__ __forceinline__ UfTap uf_tap(int i, int n2) {
    const float p = fminf(fmaxf(0.5f * (float)i - 0.25f, 0.0f), (float)(n2 - 1));
    UfTap a;
    a.i0 = min((int)p, max(n2 - 2, 0));
    a.i1 = min(a.i0 + 1, n2 - 1);
    a.t = p - (float)a.i0;
    return a;
}

// the weight of coarse texel j among fine texel i's taps on one axis
__device__ __forceinline__ float uf_tap_weight(int i, int j, int n2) {
    const UfTap a = uf_tap(i, n2);
    return (a.i0 == j ? 1.0f - a.t : 0.0f) + (a.i1 == j ? a.t : 0.0f);
}

__device__ __forceinline__ float uf_up(float c00, float c01, float c10, float c11, float tx, float ty) {
    return (1.0f - ty) * ((1.0f - tx) * c00 + tx * c01) + ty * ((1.0f - tx) * c10 + tx * c11);
}

// ---- forward 1: fusion and the pull inside a tile -------------------------------------------------------------------------------
// One workgroup per 32 x 32 level-0 tile (clipped to the image), the channels in chunks of UVT_CHUNK, lanes along the tile rows'
// contiguous (x, c) axis.  valid is written everywhere, the output at valid texels (without the fill: everywhere); (s, n) of
// levels 1..min(L, 5) are built in LDS and stored.
__global__ void __launch_bounds__(256) k_uv_fill_fuse_tile(const float* __restrict__ textures, const float* __restrict__ weights,
                                                          int B, UvFill uf, int fill, const float* __restrict__ background,
                                                          float* __restrict__ out, float* __restrict__ valid,
                                                          float* __restrict__ sums, int* __restrict__ counts) {
    __shared__ float s_sum[UVT_TILE_TEXELS * UVT_CHUNK];
    __shared__ int s_cnt[UVT_TILE_TEXELS];
    const int H = uf.H, W = uf.W, C = uf.C;
    const int tiles_x = (W + UVT_TILE - 1) / UVT_TILE;
    const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
    const int x0 = tx * UVT_TILE, y0 = ty * UVT_TILE;
    const int tw = min(UVT_TILE, W - x0), th = min(UVT_TILE, H - y0);
    const int lt = min(uf.L, UVT_TILE_LEVELS);
    const size_t plane = (size_t)H * W;
    for (int e = threadIdx.x; e < th * tw; e += 256) {
        const int y = e / tw, x = e - y * tw;
        const size_t at = (size_t)(y0 + y) * W + x0 + x;
        bool v = false;
        for (int b = 0; b < B; b++) v = v || weights[b * plane + at] > 0.0f;
        s_cnt[e] = v ? 1 : 0;
        valid[at] = v ? 1.0f : 0.0f;
    }
    __syncthreads();
    for (int k0 = 0; k0 < C; k0 += UVT_CHUNK) {
        const int cc = min(UVT_CHUNK, C - k0), row = tw * cc;
        for (int e = threadIdx.x; e < th * row; e += 256) {
            const int y = e / row, r = e - y * row, x = r / cc, k = r - x * cc;
            const size_t at = (size_t)(y0 + y) * W + x0 + x;
            float v = 0.0f;
            if (s_cnt[y * tw + x]) {
                float a = 0.0f, m = 0.0f;
                bool first = true;
                for (int b = 0; b < B; b++) {
                    const float w = weights[b * plane + at];
                    if (!(w > 0.0f)) continue;
                    const float term = w * textures[(b * plane + at) * C + k0 + k];
                    a = first ? term : a + term;
                    m = first ? w : m + w;
                    first = false;
                }
                v = a / m;
                out[at * C + k0 + k] = v;
            } else if (!fill) {
                out[at * C + k0 + k] = background ? background[k0 + k] : 0.0f;
            }
            s_sum[e] = v;
        }
        if (!fill) continue;                                            // (uniform: nothing below is needed)
        __syncthreads();
        int base = 0;                                                   // level l - 1's first texel in s_sum / s_cnt
        for (int l = 1; l <= lt; l++) {
            const int wp = uf_size(tw, l - 1), hp = uf_size(th, l - 1), wl = uf_size(tw, l), hl = uf_size(th, l);
            const int next = base + hp * wp, Wl = uf_size(W, l);
            for (int e = threadIdx.x; e < hl * wl * cc; e += 256) {
                const int y = e / (wl * cc), r = e - y * wl * cc, x = r / cc, k = r - x * cc;
                const bool right = 2 * x + 1 < wp, down = 2 * y + 1 < hp;
                const int c00 = base + 2 * y * wp + 2 * x;
                const float* a = s_sum + c00 * cc + k;
                const float v = ((a[0] + (right ? a[cc] : 0.0f)) + (down ? a[wp * cc] : 0.0f)) +
                                (right && down ? a[(wp + 1) * cc] : 0.0f);
                s_sum[(next + y * wl + x) * cc + k] = v;
                const size_t at = uf.offset[l] + (size_t)((y0 >> l) + y) * Wl + (x0 >> l) + x;
                sums[at * C + k0 + k] = v;
                if (k0 == 0 && k == 0) {
                    const int* q = s_cnt + c00;
                    const int n = ((q[0] + (right ? q[1] : 0)) + (down ? q[wp] : 0)) + (right && down ? q[wp + 1] : 0);
                    s_cnt[next + y * wl + x] = n;
                    counts[at] = n;
                }
            }
            __syncthreads();
            base = next;
        }
    }
}

// ---- forward 2: the levels above the tiles, up and back down ----------------------------------------------------------------------
// One workgroup: (s, n) of levels 6..L, each from the one below it in the pyramids, then f_L and f of levels L - 1..min(L, 5)
// into `top` (level l at texel offset[l] - offset[min(L, 5)]; the 1 x 1 image: one texel).  Lanes along the (x, c) axis.
__device__ __forceinline__ long uf_top_offset(const UvFill& uf, int l) {
    const int lt = min(uf.L, UVT_TILE_LEVELS);
    return lt == 0 ? 0 : uf.offset[l] - uf.offset[lt];
}

__global__ void __launch_bounds__(UF_TOP_BLOCK) k_uv_fill_top(UvFill uf, const float* __restrict__ background, const float* out,
                                                             const float* valid, float* sums, int* counts, float* top) {
    const int C = uf.C, L = uf.L, lt = min(L, UVT_TILE_LEVELS);
    for (int l = lt + 1; l <= L; l++) {                                 // (lt = 5 here: the source is in the pyramids)
        const int wp = uf_size(uf.W, l - 1), hp = uf_size(uf.H, l - 1), wl = uf_size(uf.W, l), hl = uf_size(uf.H, l);
        const float* src = sums + (size_t)uf.offset[l - 1] * C;
        const int* src_n = counts + uf.offset[l - 1];
        float* dst = sums + (size_t)uf.offset[l] * C;
        const long row = (long)wl * C, n_el = (long)hl * row;
        for (long e = threadIdx.x; e < n_el; e += UF_TOP_BLOCK) {
            const int y = (int)(e / row), r = (int)(e - (long)y * row), x = r / C, k = r - x * C;
            const bool right = 2 * x + 1 < wp, down = 2 * y + 1 < hp;
            const size_t c00 = (size_t)2 * y * wp + 2 * x;
            const float* a = src + c00 * C + k;
            dst[e] = ((a[0] + (right ? a[C] : 0.0f)) + (down ? a[(size_t)wp * C] : 0.0f)) +
                     (right && down ? a[((size_t)wp + 1) * C] : 0.0f);
            if (k == 0) {
                const int* q = src_n + c00;
                counts[uf.offset[l] + (long)y * wl + x] =
                    ((q[0] + (right ? q[1] : 0)) + (down ? q[wp] : 0)) + (right && down ? q[wp + 1] : 0);
            }
        }
        __threadfence();                                                // the next level reads what other lanes stored
        __syncthreads();
    }
    for (int l = L; l >= lt; l--) {
        const int wl = uf_size(uf.W, l), hl = uf_size(uf.H, l), w2 = uf_size(uf.W, l + 1), h2 = uf_size(uf.H, l + 1);
        float* f = top + (size_t)uf_top_offset(uf, l) * C;
        const float* coarse = l < L ? top + (size_t)uf_top_offset(uf, l + 1) * C : nullptr;
        const long row = (long)wl * C, n_el = (long)hl * row;
        for (long e = threadIdx.x; e < n_el; e += UF_TOP_BLOCK) {
            const int y = (int)(e / row), r = (int)(e - (long)y * row), x = r / C, k = r - x * C;
            const long at = (long)y * wl + x;
            const int n = l == 0 ? (valid[at] > 0.0f ? 1 : 0) : counts[uf.offset[l] + at];
            float v;
            if (n > 0) {
                v = (l == 0 ? out[at * C + k] : sums[(size_t)(uf.offset[l] + at) * C + k]) / (float)n;
            } else if (l == L) {
                v = background ? background[k] : 0.0f;
            } else {
                const UfTap ay = uf_tap(y, h2), ax = uf_tap(x, w2);
                v = uf_up(coarse[((size_t)ay.i0 * w2 + ax.i0) * C + k], coarse[((size_t)ay.i0 * w2 + ax.i1) * C + k],
                          coarse[((size_t)ay.i1 * w2 + ax.i0) * C + k], coarse[((size_t)ay.i1 * w2 + ax.i1) * C + k], ax.t, ay.t);
            }
            f[e] = v;
        }
        __threadfence();
        __syncthreads();
    }
}

// ---- forward 3: the push inside a tile ----------------------------------------------------------------------------------------------
// One workgroup per 32 x 32 level-0 tile.  At level l = min(L, 5)..1 it holds f_l in LDS on the tile's texels of that level and a
// halo of one around them (clipped to the level; recomputed per tile): level min(L, 5) from `top`, the others from (s, n) of the
// pyramids and the level above in LDS.  A fine texel 2j takes the coarse taps j - 1 and j, 2j + 1 takes j and j + 1, and the
// tile's first texel of every level is even: the halo of one holds every tap.  Level 0: the invalid texels are stored.
__global__ void __launch_bounds__(256) k_uv_fill_push_tile(UvFill uf, const float* __restrict__ valid,
                                                          const float* __restrict__ sums, const int* __restrict__ counts,
                                                          const float* __restrict__ top, float* __restrict__ out) {
    __shared__ float s_f[2][UF_PUSH_WINDOW * UVT_CHUNK];
    const int W = uf.W, H = uf.H, C = uf.C;
    const int tiles_x = (W + UVT_TILE - 1) / UVT_TILE;
    const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
    const int x0 = tx * UVT_TILE, y0 = ty * UVT_TILE;
    const int lt = min(uf.L, UVT_TILE_LEVELS);
    for (int k0 = 0; k0 < C; k0 += UVT_CHUNK) {
        const int cc = min(UVT_CHUNK, C - k0);
        for (int l = lt; l >= 0; l--) {
            const int wl = uf_size(W, l), hl = uf_size(H, l), side = UVT_TILE >> l, halo = l > 0 ? 1 : 0;
            const int ox = (x0 >> l) - halo, oy = (y0 >> l) - halo, ww = side + 2 * halo;           // the window: origin, width
            const int lo_x = max(ox, 0), lo_y = max(oy, 0), rw = min(ox + ww, wl) - lo_x, rh = min(oy + ww, hl) - lo_y;
            const int w2 = uf_size(W, l + 1), h2 = uf_size(H, l + 1);                               // the level above, in LDS
            const int ox2 = (x0 >> (l + 1)) - 1, oy2 = (y0 >> (l + 1)) - 1, ww2 = (UVT_TILE >> (l + 1)) + 2;
            const float* coarse = s_f[(l + 1) & 1];
            float* fine = s_f[l & 1];
            for (int e = threadIdx.x; e < rh * rw * cc; e += 256) {
                const int y = e / (rw * cc), r = e - y * rw * cc, x = r / cc, k = r - x * cc;
                const int gy = lo_y + y, gx = lo_x + x;
                const size_t at = (size_t)gy * wl + gx;
                const int n = l == 0 ? (valid[at] > 0.0f ? 1 : 0) : counts[uf.offset[l] + at];
                if (l == 0 && n > 0) continue;                          // written by k_uv_fill_fuse_tile
                float v;
                if (l == lt) {
                    v = top[at * C + k0 + k];
                } else if (n > 0) {
                    v = sums[(uf.offset[l] + at) * C + k0 + k] / (float)n;
                } else {
                    const UfTap ay = uf_tap(gy, h2), ax = uf_tap(gx, w2);
                    const int r0 = (ay.i0 - oy2) * ww2, r1 = (ay.i1 - oy2) * ww2, c0 = ax.i0 - ox2, c1 = ax.i1 - ox2;
                    v = uf_up(coarse[(r0 + c0) * cc + k], coarse[(r0 + c1) * cc + k], coarse[(r1 + c0) * cc + k],
                              coarse[(r1 + c1) * cc + k], ax.t, ay.t);
                }
                if (l == 0) out[at * C + k0 + k] = v;
                else fine[((gy - oy) * ww + gx - ox) * cc + k] = v;
            }
            __syncthreads();
        }
    }
}

// ---- backward 1: the push adjoint, fine to coarse ---------------------------------------------------------------------------------
// G of levels base + 1..base + steps from G of level `base` (base = 0: the output gradient), one workgroup per 32 x 32 tile of
// level `base`.  Step s has its own texels [a >> s, b >> s) and a halo of h_s = 2 (2^(steps - s) - 1) around them, clipped to the
// level and recomputed per tile: G(j) reads the fine texels 2j - 2..2j + 3, so h_{s-1} = 2 h_s + 2 holds them.  Step 1 reads
// level `base` from memory; the later steps read the step before in LDS, kept as n == 0 ? G : 0 (a valid texel passes nothing
// up).  The own texels of every step are stored.  steps <= UF_ADJ_STEPS, or the whole level `base` is one tile (steps <= 5):
// then every window is a whole level of at most 16 x 16.
__global__ void __launch_bounds__(256) k_uv_fill_adjoint_tile(UvFill uf, int base, int steps, const float* __restrict__ grad_out,
                                                             const float* __restrict__ valid, const int* __restrict__ counts,
                                                             float* __restrict__ G) {
    __shared__ float s_a[UF_ADJ_WINDOW_A * UVT_CHUNK];
    __shared__ float s_b[UF_ADJ_WINDOW_B * UVT_CHUNK];
    const int C = uf.C;
    const int wb = uf_size(uf.W, base), hb = uf_size(uf.H, base);
    const int tiles_x = (wb + UVT_TILE - 1) / UVT_TILE;
    const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
    const int x0 = tx * UVT_TILE, y0 = ty * UVT_TILE;
    const float* g_base = base == 0 ? grad_out : G + (size_t)uf.offset[base] * C;
    for (int k0 = 0; k0 < C; k0 += UVT_CHUNK) {
        const int cc = min(UVT_CHUNK, C - k0);
        int p_lo_x = 0, p_lo_y = 0, p_rw = 0;                           // the window of the step before
        for (int s = 1; s <= steps; s++) {
            const int l = base + s, wl = uf_size(uf.W, l), hl = uf_size(uf.H, l);
            const int wp = uf_size(uf.W, l - 1), hp = uf_size(uf.H, l - 1);
            const int h = 2 * ((1 << (steps - s)) - 1);
            const int ax = x0 >> s, ay = y0 >> s, bx = min((x0 + UVT_TILE) >> s, wl), by = min((y0 + UVT_TILE) >> s, hl);
            const int lo_x = max(ax - h, 0), lo_y = max(ay - h, 0), rw = min(bx + h, wl) - lo_x, rh = min(by + h, hl) - lo_y;
            float* cur = (s & 1) ? s_a : s_b;
            const float* prev = (s & 1) ? s_b : s_a;
            if (s < steps && rw * rh > ((s & 1) ? UF_ADJ_WINDOW_A : UF_ADJ_WINDOW_B)) return;      // (uniform; the host's plan keeps to it)
            for (int e = threadIdx.x; e < rh * rw * cc; e += 256) {
                const int y = e / (rw * cc), r = e - y * rw * cc, x = r / cc, k = r - x * cc;
                const int jy = lo_y + y, jx = lo_x + x;
                const int iy0 = max(2 * jy - 2, 0), ix0 = max(2 * jx - 2, 0);
                float wy[6], wx[6];
#pragma unroll
                for (int d = 0; d < 6; d++) {
                    wy[d] = iy0 + d < hp ? uf_tap_weight(iy0 + d, jy, hl) : 0.0f;
                    wx[d] = ix0 + d < wp ? uf_tap_weight(ix0 + d, jx, wl) : 0.0f;
                }
                float sum = 0.0f;
#pragma unroll
                for (int dy = 0; dy < 6; dy++) {
                    if (wy[dy] == 0.0f) continue;
                    const int iy = iy0 + dy;
#pragma unroll
                    for (int dx = 0; dx < 6; dx++) {
                        const float w = wy[dy] * wx[dx];
                        if (w == 0.0f) continue;
                        const int ix = ix0 + dx;
                        float v;
                        if (s == 1) {
                            const size_t at = (size_t)iy * wb + ix;
                            const bool filled = base == 0 ? !(valid[at] > 0.0f) : counts[uf.offset[base] + at] == 0;
                            if (!filled) continue;
                            v = g_base[at * C + k0 + k];
                        } else {
                            v = prev[((iy - p_lo_y) * p_rw + ix - p_lo_x) * cc + k];
                        }
                        sum += w * v;
                    }
                }
                const size_t at = uf.offset[l] + (size_t)jy * wl + jx;
                if (jy >= ay && jy < by && jx >= ax && jx < bx) G[at * C + k0 + k] = sum;
                if (s < steps) cur[e] = counts[at] == 0 ? sum : 0.0f;
            }
            __syncthreads();
            p_lo_x = lo_x;
            p_lo_y = lo_y;
            p_rw = rw;
        }
    }
}

// ---- backward 2: the pull and the fusion adjoint ----------------------------------------------------------------------------------
// One lane per element (t, k) of the output gradient (a grid striding over them), every view's element written.  levels = L with
// the fill, 0 without it (gs_0 = g).
__global__ void __launch_bounds__(256) k_uv_fill_adjoint_views(UvFill uf, int B, int levels, const float* __restrict__ weights,
                                                              const float* __restrict__ valid, const int* __restrict__ counts,
                                                              const float* __restrict__ G, const float* __restrict__ grad_out,
                                                              float* __restrict__ grad_textures) {
    const int W = uf.W, C = uf.C;
    const size_t plane = (size_t)uf.H * W, n_el = plane * C;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n_el; i += (size_t)gridDim.x * 256) {
        const size_t t = i / C;
        const int k = (int)(i - t * C), y = (int)(t / W), x = (int)(t - (size_t)y * W);
        const bool v = valid[t] > 0.0f;
        float gs = 0.0f, m = 0.0f;
        if (v) {
            bool first = true;
            for (int l = levels; l >= 1; l--) {
                const size_t at = uf.offset[l] + (size_t)(y >> l) * uf_size(W, l) + (x >> l);
                const float term = G[at * C + k] / (float)counts[at];
                gs = first ? term : gs + term;
                first = false;
            }
            gs = first ? grad_out[i] : gs + grad_out[i];
            first = true;
            for (int b = 0; b < B; b++) {
                const float w = weights[b * plane + t];
                if (!(w > 0.0f)) continue;
                m = first ? w : m + w;
                first = false;
            }
        }
        for (int b = 0; b < B; b++) {
            const float w = weights[b * plane + t];
            grad_textures[b * n_el + i] = v && w > 0.0f ? (w / m) * gs : 0.0f;
        }
    }
}

}  // namespace d3m
