// d3m_attributes.h -- per-vertex attribute images: C channels of per-vertex data (positions, normals, codes, uv, features)
// interpolated over a coverage record (face_index_map / weight_map / depth_map and the dense screen-space faces that
// d3m_forward_face_index_map_mesh leaves) into images [B, C, s, s], and the adjoint with respect to the attributes.
//
// Internal pixel p of view b with owner fn >= 0: f = fn mod F, corner c of the owner is vertex tri[f][c] (fn < F) or
// tri[f][2 - c] (the fill_back copy), u_c = weight_map[b,p,c] * (depth_map[b,p] / faces[b,fn,c,2]) -- the sampler's
// perspective-correct weights (sample_setup, d3m_lit.h) -- and value[k] = (u_0 a_0[k] + u_1 a_1[k]) + u_2 a_2[k]; an
// uncovered pixel takes background[k].  The output image is what the output epilogue (k_output_epilogue) makes of such a
// map: rows reversed and, with anti-aliasing, s = 0; s += value(2 yo + dy, 2 xo + dx) for (dy, dx) = (0,0), (0,1), (1,0),
// (1,1) in OUTPUT orientation; s * 0.25.  alpha is the coverage (1 / 0) treated the same way.
//
// THE ORDER of the adjoint's sums, the same bits on every run (no float atomics anywhere, nothing is cleared):
//   1. per visible face (b, fn), channel k, corner c:  G[b,fn,c,k] = sum over the pixels p the face owns of
//      u_c(p) * (scale * g[b,k,out(p)]), scale = 1 or 1/4, out(p) the output pixel that internal pixel p feeds.  Route and
//      order: stage 1 of d3m_fragments.h (THE ORDER there), with 3 * VA_CHUNK accumulators a face and channel chunk.
//      G [B,F',3,C] is stored plainly; entries of faces that own no pixel are never written and never read.
//   2. per vertex v, channel k (and view b, or -- shared attributes -- one accumulator over b = 0, 1, ... in that order):
//      acc = 0; for the items 3 f + c of the vertex's adjacency row in ascending order: acc += G[b,f,c,k] if face f is
//      visible in view b, then -- fill_back -- acc += G[b,F+f,2-c,k] if the copy is.  A row of more than long_row items goes
//      through the chunks of d3m_row_gather.h (steps 1 to 4, an item's term being the sum of those two entries, 0 + front +
//      copy), the chunk sums of view b added in chunk order.  A vertex of no face, or of no visible face, gets an exact +0.
#pragma once
#include "d3m_fragments.h"

namespace d3m {

constexpr int VA_MAX_CHANNELS = 1024;

// ---- forward: fr_output_pixel_walk (d3m_fragments.h) over the owner's three corner vertices and their weights ---------------
__global__ void __launch_bounds__(256) k_vertex_attribute_images(AttrMaps m, const float* __restrict__ attributes,
                                                                int attr_batch, int V, int C,
                                                                const float* __restrict__ background,
                                                                float* __restrict__ images, float* __restrict__ alpha) {
    const float* attr = attributes + (size_t)(attr_batch > 1 ? (int)blockIdx.y : 0) * V * C;
    int ids[4][3];
    float u[4][3];
    fr_output_pixel_walk(
        m, C, background, images, alpha,
        [&](int j, int b, size_t q, int fn) {
            const bool back = fn >= m.Ft;
            const int32_t* t = m.tri + (size_t)(back ? fn - m.Ft : fn) * 3;
            float z[3];
            fr_corner_depths(m, b, fn, z);
            va_weights(m, q, z, u[j]);
            ids[j][0] = back ? t[2] : t[0];
            ids[j][1] = t[1];
            ids[j][2] = back ? t[0] : t[2];
        },
        [&](int j, int k) {
            return (u[j][0] * attr[(size_t)ids[j][0] * C + k] + u[j][1] * attr[(size_t)ids[j][1] * C + k]) +
                   u[j][2] * attr[(size_t)ids[j][2] * C + k];
        });
}

// ---- adjoint, stage 1: fr_face_sums / fr_large_face_sums (d3m_fragments.h), blockIdx.y = the channel chunk -----------------
struct VaFaceSums {
    const AttrMaps& m;
    const float* grad_images;
    int C, k0;
    float* G;
    float z[3];
    const float* g_view;
    __device__ __forceinline__ void setup(const float* face, int b) {
        const int s = fr_output_size(m);
        fr_corner_depths(face, z);
        g_view = grad_images + (size_t)b * C * s * s;
    }
    __device__ __forceinline__ void add(int x, int y, size_t q, float* acc) const {
        float u[3], gs[VA_CHUNK];
        va_weights(m, q, z, u);
        va_pixel_grads(m, g_view, C, k0, x, y, gs);
#pragma unroll
        for (int c = 0; c < 3; c++)
#pragma unroll
            for (int kk = 0; kk < VA_CHUNK; kk++) acc[c * VA_CHUNK + kk] += u[c] * gs[kk];
    }
    __device__ __forceinline__ void store(size_t gi, const float* acc) const {
#pragma unroll
        for (int c = 0; c < 3; c++)
#pragma unroll
            for (int kk = 0; kk < VA_CHUNK; kk++)
                if (k0 + kk < C) G[(gi * 3 + c) * C + k0 + kk] = acc[c * VA_CHUNK + kk];
    }
};

__global__ void __launch_bounds__(256) k_vertex_attribute_face_sums(AttrMaps m, const float* __restrict__ grad_images, int C,
                                                                   const int* __restrict__ list,
                                                                   const int* __restrict__ n_list, float* __restrict__ G) {
    VaFaceSums policy{m, grad_images, C, (int)blockIdx.y * VA_CHUNK, G};
    fr_face_sums<3 * VA_CHUNK>(m, list, n_list, policy);
}

__global__ void __launch_bounds__(RG_BLOCK) k_vertex_attribute_large_face_sums(AttrMaps m, const float* __restrict__ grad_images,
                                                                              int C, const int* __restrict__ list,
                                                                              const int* __restrict__ n_list,
                                                                              float* __restrict__ G) {
    VaFaceSums policy{m, grad_images, C, (int)blockIdx.y * VA_CHUNK, G};
    fr_large_face_sums<3 * VA_CHUNK>(m, list, n_list, policy);
}

// ---- adjoint, stage 2: the gather over the faces' adjacency ---------------------------------------------------------------
// an item's entries of view b, channel k: the front face's and, with fill_back, the copy's -- each only if it owns a pixel
__device__ __forceinline__ void va_add_item(const float* __restrict__ G, const int* __restrict__ flags, int Ft, int Fp, int C,
                                            int b, int item, int k, float& acc) {
    const int f = item / 3, c = item - 3 * f;
    const size_t view = (size_t)b * Fp;
    if (flags[view + f] != FLAG_HIDDEN) acc += G[((view + f) * 3 + c) * C + k];
    if (Fp > Ft && flags[view + Ft + f] != FLAG_HIDDEN) acc += G[((view + Ft + f) * 3 + (2 - c)) * C + k];
}

// the chunk sums of the long rows: partials [B, n_chunks, C]; blockIdx = (chunk, view, channel chunk)
__global__ void __launch_bounds__(RG_BLOCK) k_vertex_attribute_adjoint_chunks(const int32_t* __restrict__ adj_items,
                                                                             const int2* __restrict__ chunks, int n_chunks,
                                                                             const float* __restrict__ G,
                                                                             const int* __restrict__ flags, int Ft, int Fp,
                                                                             int C, float* __restrict__ partials) {
    const int ch = blockIdx.x, b = blockIdx.y, k0 = blockIdx.z * VA_CHUNK;
    float sum[VA_CHUNK];
    rg_chunk_sum(chunks[ch], sum, [&](int e, float (&acc)[VA_CHUNK]) {
        const int item = adj_items[e];
#pragma unroll
        for (int kk = 0; kk < VA_CHUNK; kk++) {
            if (k0 + kk >= C) continue;
            float term = 0.0f;
            va_add_item(G, flags, Ft, Fp, C, b, item, k0 + kk, term);
            acc[kk] += term;
        }
    });
    if (threadIdx.x == 0) {
        float* out = partials + ((size_t)b * n_chunks + ch) * C;
#pragma unroll
        for (int kk = 0; kk < VA_CHUNK; kk++)
            if (k0 + kk < C) out[k0 + kk] = sum[kk];
    }
}

// One lane per element (v, k) of grad_attributes; blockIdx.y = the view when the attributes are per view, else the lane
// goes over the views itself.  Every element is written.
__global__ void __launch_bounds__(256) k_vertex_attribute_adjoint_rows(CsrRows adj, const float* __restrict__ partials,
                                                                      const float* __restrict__ G,
                                                                      const int* __restrict__ flags, int B, int Ft, int Fp,
                                                                      int V, int C, int shared,
                                                                      float* __restrict__ grad_attributes) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long)V * C) return;
    const int v = (int)(i / C), k = (int)(i - (long)v * C);
    const int start = adj.offsets[v], end = adj.offsets[v + 1];
    const bool is_long = rg_is_long(adj.longs, end - start);
    const int l = is_long ? rg_find_long(adj.longs, v) : 0;
    const int b0 = shared ? 0 : blockIdx.y, b1 = shared ? B : b0 + 1;
    float acc = 0.0f;
    for (int b = b0; b < b1; b++) {
        if (is_long) {
            const float* part = partials + (size_t)b * adj.longs.n_chunks * C + k;
            for (int c = adj.longs.chunk_ptr[l]; c < adj.longs.chunk_ptr[l + 1]; c++) acc += part[(size_t)c * C];
        } else {
            for (int e = start; e < end; e++) va_add_item(G, flags, Ft, Fp, C, b, adj.items[e], k, acc);
        }
    }
    grad_attributes[(size_t)(shared ? 0 : b0) * V * C + i] = acc;
}

}  // namespace d3m
