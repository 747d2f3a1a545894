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
//      u_c(p) * (scale * g[b,k,out(p)]), scale = 1 or 1/4, out(p) the output pixel that internal pixel p feeds.
//      a. a face whose clipped box has at most FM_MAX_BBOX_AREA pixels: FM_LANES lanes share scan_owned_pixels
//         (d3m_face_major.h): the owned pixels are numbered in ascending box order, lane `sub` adds those of rank sub,
//         sub + FM_LANES, ... in that order from 0, and the lanes are combined by quad_sum (lane ^ 1, lane ^ 2, then the
//         other quad of the eight);
//      b. a larger face: one workgroup of RG_BLOCK lanes; lane t adds the owned pixels among box pixels t, t + RG_BLOCK,
//         ... (row-major in the box) in that order from 0, and the lanes are combined by rg_block_sum (d3m_row_gather.h,
//         steps 2 and 3).
//      G is stored plainly; entries of faces that own no pixel are never written and never read.
//   2. per vertex v, channel k (and view b, or -- shared attributes -- one accumulator over b = 0, 1, ... in that order):
//      acc = 0; for the items 3 f + c of the vertex's adjacency row in ascending order: acc += G[b,f,c,k] if face f is
//      visible in view b, then -- fill_back -- acc += G[b,F+f,2-c,k] if the copy is.  A row of more than long_row items goes
//      through the chunks of d3m_row_gather.h (steps 1 to 4, an item's term being the sum of those two entries, 0 + front +
//      copy), the chunk sums of view b added in chunk order.  A vertex of no face, or of no visible face, gets an exact +0.
#pragma once
#include "d3m_face_major.h"
#include "d3m_row_gather.h"

namespace d3m {

constexpr int VA_CHUNK = 8;          // channels a lane keeps in registers at a time (attributes.CHANNEL_CHUNK)
constexpr int VA_MAX_CHANNELS = 1024;

// A coverage record as the kernels read it (row 0 of the maps = bottom).
struct AttrMaps {
    const int32_t* face_index_map;   // [B,S,S]
    const float* weight_map;         // [B,S,S,3]
    const float* depth_map;          // [B,S,S]
    const float* faces;              // [B,Fp,3,3] the dense copy: only owners' entries are defined, only those are read
    const int32_t* tri;              // [Ft,3]
    int B, S, Ft, Fp, aa;
};

// u_c of internal pixel q (index into the batch's maps) owned by a face whose corner depths are z[0..2]
__device__ __forceinline__ void va_weights(const AttrMaps& m, size_t q, const float* z, float* u) {
    const float d = m.depth_map[q];
#pragma unroll
    for (int c = 0; c < 3; c++) u[c] = m.weight_map[3 * q + c] * (d / z[c]);
}

// ---- forward: one lane per OUTPUT pixel; the 1 or 4 internal pixels' owners, weights and vertices are gathered once and the
// channels walked in chunks of VA_CHUNK (registers do not grow with C); adjacent lanes store adjacent pixels of one
// channel plane.  Every element of images and alpha is written.
__global__ void __launch_bounds__(256) k_vertex_attribute_images(AttrMaps m, const float* __restrict__ attributes,
                                                                int attr_batch, int V, int C,
                                                                const float* __restrict__ background,
                                                                float* __restrict__ images, float* __restrict__ alpha) {
    const int s = m.aa ? m.S / 2 : m.S;
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    const int b = blockIdx.y;
    if (i >= (long)s * s) return;
    const int yo = (int)(i / s), xo = (int)(i - (long)yo * s);
    const int np = m.aa ? 4 : 1;
    int ids[4][3];
    float u[4][3];
    bool covered[4];
    float n_cov = 0.0f;
    const float* attr = attributes + (size_t)(attr_batch > 1 ? b : 0) * V * C;
#pragma unroll
    for (int j = 0; j < 4; j++) {
        covered[j] = false;
        if (j >= np) continue;
        const int yi = m.S - 1 - (m.aa ? 2 * yo + (j >> 1) : yo), xi = m.aa ? 2 * xo + (j & 1) : xo;
        const size_t q = ((size_t)b * m.S + yi) * m.S + xi;
        const int fn = m.face_index_map[q];
        if ((unsigned)fn >= (unsigned)m.Fp) continue;                   // uncovered (-1)
        const bool back = fn >= m.Ft;
        const int32_t* t = m.tri + (size_t)(back ? fn - m.Ft : fn) * 3;
        const float* face = m.faces + ((size_t)b * m.Fp + fn) * 9;
        const float z[3] = {face[2], face[5], face[8]};
        va_weights(m, q, z, u[j]);
        ids[j][0] = back ? t[2] : t[0];
        ids[j][1] = t[1];
        ids[j][2] = back ? t[0] : t[2];
        covered[j] = true;
        n_cov += 1.0f;
    }
    const float inv = m.aa ? 0.25f : 1.0f;
    float* out = images + (size_t)b * C * s * s + i;
    for (int k0 = 0; k0 < C; k0 += VA_CHUNK) {
        float acc[VA_CHUNK];
#pragma unroll
        for (int kk = 0; kk < VA_CHUNK; kk++) acc[kk] = 0.0f;
#pragma unroll
        for (int j = 0; j < 4; j++) {
            if (j >= np) continue;
#pragma unroll
            for (int kk = 0; kk < VA_CHUNK; kk++) {
                const int k = k0 + kk;
                if (k >= C) continue;
                if (covered[j])
                    acc[kk] += (u[j][0] * attr[(size_t)ids[j][0] * C + k] + u[j][1] * attr[(size_t)ids[j][1] * C + k]) +
                               u[j][2] * attr[(size_t)ids[j][2] * C + k];
                else
                    acc[kk] += background ? background[k] : 0.0f;
            }
        }
#pragma unroll
        for (int kk = 0; kk < VA_CHUNK; kk++)
            if (k0 + kk < C) out[(size_t)(k0 + kk) * s * s] = acc[kk] * inv;
    }
    alpha[(size_t)b * s * s + i] = n_cov * inv;
}

// ---- adjoint, stage 1 ---------------------------------------------------------------------------------------------------
// scale * g[b, k0 + kk, out(x, y)] for the chunk's channels
__device__ __forceinline__ void va_pixel_grads(const AttrMaps& m, const float* __restrict__ g_view, int C, int k0, int x, int y,
                                               float* gs) {
    const int s = m.aa ? m.S / 2 : m.S;
    const int yo = m.aa ? (m.S - 1 - y) >> 1 : m.S - 1 - y, xo = m.aa ? x >> 1 : x;
    const float scale = m.aa ? 0.25f : 1.0f;
    const float* g = g_view + ((size_t)k0 * s + yo) * s + xo;
#pragma unroll
    for (int kk = 0; kk < VA_CHUNK; kk++) gs[kk] = k0 + kk < C ? scale * g[(size_t)kk * s * s] : 0.0f;
}

// 1a: FM_LANES lanes per listed face, blockIdx.y = the channel chunk; a fixed grid strides over the visibility list
__global__ void __launch_bounds__(256) k_vertex_attribute_face_sums(AttrMaps m, const float* __restrict__ grad_images, int C,
                                                                   const int* __restrict__ list,
                                                                   const int* __restrict__ n_list, float* __restrict__ G) {
    const int sub = threadIdx.x % FM_LANES;
    const int k0 = blockIdx.y * VA_CHUNK;
    const int s = m.aa ? m.S / 2 : m.S;
    const long n_units = min((long)*n_list, (long)m.B * m.Fp);      // (the list has one entry per face at most)
    for (long un = (long)blockIdx.x * FM_FACES_PER_BLOCK + threadIdx.x / FM_LANES; un < n_units;
         un += (long)gridDim.x * FM_FACES_PER_BLOCK) {
        const long gi = list[un];
        if (gi < 0 || gi >= (long)m.B * m.Fp) continue;
        const int bn = (int)(gi / m.Fp), fn = (int)(gi - (long)bn * m.Fp);
        float face[9];
#pragma unroll
        for (int k = 0; k < 9; k++) face[k] = m.faces[(size_t)gi * 9 + k];
        int x0 = 0, x1 = 0, y0 = 0, y1 = 0;
        const bool boxed = pixel_bbox(face, m.S, x0, x1, y0, y1);
        const int area = boxed ? (x1 - x0 + 1) * (y1 - y0 + 1) : 0;
        if (area > FM_MAX_BBOX_AREA) continue;                          // 1b's
        float acc[3][VA_CHUNK];
#pragma unroll
        for (int c = 0; c < 3; c++)
#pragma unroll
            for (int kk = 0; kk < VA_CHUNK; kk++) acc[c][kk] = 0.0f;
        const size_t base = (size_t)bn * m.S * m.S;
        const float z[3] = {face[2], face[5], face[8]};
        const float* g_view = grad_images + (size_t)bn * C * s * s;
        if (boxed)
            scan_owned_pixels<FM_LANES>(m.face_index_map + base, fn, m.S, x0, x1, y0, area, sub, [&](int x, int y) {
                float u[3], gs[VA_CHUNK];
                va_weights(m, base + (size_t)y * m.S + x, z, u);
                va_pixel_grads(m, g_view, C, k0, x, y, gs);
#pragma unroll
                for (int c = 0; c < 3; c++)
#pragma unroll
                    for (int kk = 0; kk < VA_CHUNK; kk++) acc[c][kk] += u[c] * gs[kk];
            });
#pragma unroll
        for (int c = 0; c < 3; c++)
#pragma unroll
            for (int kk = 0; kk < VA_CHUNK; kk++) acc[c][kk] = quad_sum(acc[c][kk]);
        if (sub == 0) {
#pragma unroll
            for (int c = 0; c < 3; c++)
#pragma unroll
                for (int kk = 0; kk < VA_CHUNK; kk++)
                    if (k0 + kk < C) G[((size_t)gi * 3 + c) * C + k0 + kk] = acc[c][kk];
        }
    }
}

// 1b: the listed faces whose box exceeds FM_MAX_BBOX_AREA, a workgroup per face.  A workgroup takes RG_BLOCK list entries
// at a time: lane t looks at entry base + t and notes it when it is large; the workgroup then walks the noted faces one
// after another (which workgroup meets which face does not matter: every face's sums are its own).
__global__ void __launch_bounds__(RG_BLOCK) k_vertex_attribute_large_face_sums(AttrMaps m, const float* __restrict__ grad_images,
                                                                              int C, const int* __restrict__ list,
                                                                              const int* __restrict__ n_list,
                                                                              float* __restrict__ G) {
    __shared__ int s_large[RG_BLOCK];
    const int k0 = blockIdx.y * VA_CHUNK;
    const int s = m.aa ? m.S / 2 : m.S;
    const long n_units = min((long)*n_list, (long)m.B * m.Fp);      // (the list has one entry per face at most)
    const int t = threadIdx.x;
    for (long first = (long)blockIdx.x * RG_BLOCK; first < n_units; first += (long)gridDim.x * RG_BLOCK) {
        int mine = -1;
        if (first + t < n_units) {
            const long gi = list[first + t];
            if (gi >= 0 && gi < (long)m.B * m.Fp) {
                float face[9];
#pragma unroll
                for (int k = 0; k < 9; k++) face[k] = m.faces[(size_t)gi * 9 + k];
                int x0, x1, y0, y1;
                if (pixel_bbox(face, m.S, x0, x1, y0, y1) && (x1 - x0 + 1) * (y1 - y0 + 1) > FM_MAX_BBOX_AREA) mine = (int)gi;
            }
        }
        s_large[t] = mine;
        __syncthreads();
        for (int j = 0; j < RG_BLOCK; j++) {
            const int gi = s_large[j];                                  // (the same for every lane)
            if (gi < 0) continue;
            const int bn = gi / m.Fp, fn = gi - bn * m.Fp;
            float face[9];
#pragma unroll
            for (int k = 0; k < 9; k++) face[k] = m.faces[(size_t)gi * 9 + k];
            int x0, x1, y0, y1;
            pixel_bbox(face, m.S, x0, x1, y0, y1);
            const int bw = x1 - x0 + 1, area = bw * (y1 - y0 + 1);
            const size_t base = (size_t)bn * m.S * m.S;
            const float z[3] = {face[2], face[5], face[8]};
            const float* g_view = grad_images + (size_t)bn * C * s * s;
            float acc[3 * VA_CHUNK];
#pragma unroll
            for (int k = 0; k < 3 * VA_CHUNK; k++) acc[k] = 0.0f;
            for (int i = t; i < area; i += RG_BLOCK) {
                const int by = i / bw, x = x0 + (i - by * bw), y = y0 + by;
                const size_t q = base + (size_t)y * m.S + x;
                if (m.face_index_map[q] != fn) continue;
                float u[3], gs[VA_CHUNK];
                va_weights(m, q, z, u);
                va_pixel_grads(m, g_view, C, k0, x, y, gs);
#pragma unroll
                for (int c = 0; c < 3; c++)
#pragma unroll
                    for (int kk = 0; kk < VA_CHUNK; kk++) acc[c * VA_CHUNK + kk] += u[c] * gs[kk];
            }
            rg_block_sum(acc);                                          // steps 2 and 3 of d3m_row_gather.h
            if (t == 0) {
#pragma unroll
                for (int c = 0; c < 3; c++)
#pragma unroll
                    for (int kk = 0; kk < VA_CHUNK; kk++)
                        if (k0 + kk < C) G[((size_t)gi * 3 + c) * C + k0 + kk] = acc[c * VA_CHUNK + kk];
            }
            __syncthreads();                                            // (rg_block_sum's staging array is used again)
        }
        __syncthreads();
    }
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
