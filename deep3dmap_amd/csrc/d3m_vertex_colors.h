// d3m_vertex_colors.h -- learnable per-vertex colours of an indexed mesh: colours [B, V, 3] -> per-face 2x2x2 texture cubes
// [B, F, 8, 3] and the adjoint.  The cube of a face is vcolor_to_texture_cube's (deep3dmap/core/renderer/utils.py:81-94) of
// its three corner colours: the coefficient table TFI_CUBE and the association of k_textures_from_im (d3m_aux.h), so an
// image's grid mesh with faces in that kernel's corner order gets the same bits.  On the plane w0 + w1 + w2 = 1 the cube's
// trilinear sample is the barycentric mix of the corner colours: the existing sampler renders smooth colour from it.
#pragma once
#include "d3m_aux.h"
#include "d3m_row_gather.h"

namespace d3m {

// One lane per texel (f, idx) of every view: three gathered corner colours (through L2; a vertex is read by ~6 faces x 8
// texels), 12 contiguous bytes stored per lane.  The coefficients are 0, +-1/2 and 1: every product is exact, so an FMA
// contraction rounds as the separate multiply and add do.
__global__ void __launch_bounds__(256) k_vertex_color_textures(const float* __restrict__ colors,
                                                               const int32_t* __restrict__ tri,
                                                               float* __restrict__ textures, int V, long n_texels) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    const int b = blockIdx.y;
    if (i >= n_texels) return;
    const int idx = (int)(i & 7);
    const long f = i >> 3;
    const float* col = colors + (size_t)b * V * 3;
    const float* c0 = col + (size_t)tri[f * 3 + 0] * 3;
    const float* c1 = col + (size_t)tri[f * 3 + 1] * 3;
    const float* c2 = col + (size_t)tri[f * 3 + 2] * 3;
    float* o = textures + ((size_t)b * n_texels + i) * 3;
#pragma unroll
    for (int k = 0; k < 3; k++) o[k] = (TFI_CUBE[idx][0] * c0[k] + TFI_CUBE[idx][1] * c1[k]) + TFI_CUBE[idx][2] * c2[k];
}

// ---- the adjoint, gathered per vertex over the CSR adjacency d3m_vertex_gather walks (offsets [V+1], items [3F], item =
// 3 f + c in ascending order per vertex) --------------------------------------------------------------------------------
// An item's term for channel k is t = sum over idx ascending of TFI_CUBE[idx][c] * grad_textures[b, f, idx, k], from 0.
// A row of up to long_row items is ONE lane per (vertex, channel) adding its terms in item order.  A longer row (a fan
// apex, a pole) goes through the chunks of d3m_row_gather.h, which states the order: k_vertex_color_adjoint_chunks reduces
// each chunk into partials [B, n_chunks, 3], and the row's lanes add its chunk sums.  No float atomics.
constexpr int VC_ADJ_BLOCK = RG_BLOCK;

__device__ __forceinline__ float vc_item_term(const float* __restrict__ g, int item, int k) {
    const int f = item / 3, c = item - 3 * f;
    const float* gt = g + (size_t)f * 24 + k;
    float t = 0.0f;
#pragma unroll
    for (int idx = 0; idx < 8; idx++) t += TFI_CUBE[idx][c] * gt[idx * 3];
    return t;
}

__global__ void __launch_bounds__(VC_ADJ_BLOCK) k_vertex_color_adjoint_chunks(const int32_t* __restrict__ adj_items,
                                                                              const int2* __restrict__ chunks,
                                                                              int n_chunks,
                                                                              const float* __restrict__ grad_textures,
                                                                              long n_faces, float* __restrict__ partials) {
    const int ch = blockIdx.x, b = blockIdx.y;
    const float* g = grad_textures + (size_t)b * n_faces * 24;
    float sum[3];
    rg_chunk_sum(chunks[ch], sum, [&](int e, float (&acc)[3]) {
        const int item = adj_items[e];
#pragma unroll
        for (int k = 0; k < 3; k++) acc[k] += vc_item_term(g, item, k);
    });
    if (threadIdx.x == 0) {
        float* out = partials + ((size_t)b * n_chunks + ch) * 3;
        out[0] = sum[0]; out[1] = sum[1]; out[2] = sum[2];
    }
}

// One lane per element of grad_colors [B, V, 3] (the three lanes of a vertex read adjacent floats of each texel; the store
// is contiguous).  A vertex of no face has an empty row and gets 0: every element is written.
__global__ void __launch_bounds__(256) k_vertex_color_adjoint_rows(CsrRows adj, const float* __restrict__ partials,
                                                                   const float* __restrict__ grad_textures,
                                                                   long n_faces, float* __restrict__ grad_colors, int V) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    const int b = blockIdx.y;
    if (i >= (long)V * 3) return;
    const int v = (int)(i / 3), k = (int)(i - (long)v * 3);
    const int start = adj.offsets[v], end = adj.offsets[v + 1];
    float acc[1] = {0.0f};
    if (rg_is_long(adj.longs, end - start)) {
        rg_add_chunk_sums<1, 3>(adj.longs, rg_find_long(adj.longs, v), partials + (size_t)b * adj.longs.n_chunks * 3 + k, acc);
    } else {
        const float* g = grad_textures + (size_t)b * n_faces * 24;
        for (int e = start; e < end; e++) acc[0] += vc_item_term(g, adj.items[e], k);
    }
    grad_colors[(size_t)b * V * 3 + i] = acc[0];
}

}  // namespace d3m
