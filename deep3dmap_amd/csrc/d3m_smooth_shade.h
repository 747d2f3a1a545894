// d3m_smooth_shade.h -- smooth per-vertex normals of an indexed mesh, a 9-term spherical-harmonic light on per-vertex
// albedo, and the adjoint (neural_renderer/smooth_shading.py).  b = set, v = vertex, k = colour channel, j = basis term:
//
//   N_f     = (x1 - x0) x (x2 - x0)
//   s[b,v]  = sum over v's adjacency items (f, c), ascending, of N_f[b]
//   r = |s|      n = s / max(r, 1e-6)                                     (a vertex of no face: n = 0)
//   H_0 = a0   H_1 = a1 nx   H_2 = a1 ny   H_3 = a1 nz   H_4 = a2 (2 nz^2 - nx^2 - ny^2)
//   H_5 = a3 ny nz   H_6 = a3 nx nz   H_7 = a3 nx ny   H_8 = a4 (nx^2 - ny^2)
//   L[b,v,k] = sum_j sh[b,k,j] H_j(n[b,v])      shaded[b,v,k] = colors[b,v,k] L[b,v,k]
//
// and, with g = d/dshaded:
//
//   g_colors = g L     gL = g colors     g_sh[b,k,j] = sum_v gL[b,v,k] H_j(n[b,v])
//   g_n = sum_k gL_k sum_j sh[b,k,j] grad H_j(n) + g_normals
//   g_s = (g_n - n (n . g_n)) / r  where r >= 1e-6,  g_n / 1e-6 elsewhere
//   gN_f = (g_s[t0] + g_s[t1]) + g_s[t2]
//   a = x1 - x0, b = x2 - x0:   term(f,1) = b x gN   term(f,2) = gN x a   term(f,0) = -((b x gN) + (gN x a))
//   g_x[b,v] = sum over v's items, ascending, of term(item)
//
// Plain f32 VALU, 256-lane workgroups; the library's -ffp-contract=off rounds every operation once.  No float atomics, no
// workgroup waits for another: partial sums pass through a scratch array between launches.  THE ORDER of every sum:
//
//   rows (s and g_x)   a row of up to long_row items: its lane adds the items' terms in ascending item order, from 0.  A
//                      longer row: the chunk sums of d3m_row_gather.h (which states their order), added in chunk order.
//   L, g_n             j ascending from the first product; k ascending from 0; g_normals last.
//   g_sh               27 sums per set (k-major): WaveTree::DppRows, SS_BLOCK vertices per part up to SS_MAX_PARTS parts,
//                      see d3m_set_sums.h; k_smooth_shade_backward_finish is its step 4.
//   shared inputs      the gradient of an input without a set dimension is summed over the sets in ascending order by the
//                      lane that owns the element: g_colors and g_n (g_s is linear in g_n: one projection, after the last
//                      set) in k_smooth_shade_backward_vertices, g_sh in the finish (each set's sum first, then the sets).
//
// Launches.  Forward: k_smooth_shade_face_normals, k_smooth_shade_chunks<3> (long rows only), k_smooth_shade_vertices.
// Backward: k_smooth_shade_backward_vertices, k_smooth_shade_backward_finish (g_sh only), k_smooth_shade_backward_faces,
// k_smooth_shade_chunks<1> (long rows only), k_smooth_shade_backward_rows; the two chunk launches are timed as
// k_smooth_shade_normal_chunks and k_smooth_shade_term_chunks.  With shared vertices the normals and the vertex gradient are
// computed once.
#pragma once
#include "d3m_aux.h"
#include "d3m_row_gather.h"
#include "d3m_set_sums.h"

namespace d3m {

constexpr int SS_BLOCK = 256;           // lanes of a workgroup
constexpr int SS_MAX_PARTS = 64;        // workgroups per set in the per-vertex backward stage
constexpr int SS_SUMS = 27;             // g_sh of one set: 3 channels x 9 terms
constexpr float SS_EPS = 1e-6f;
// sqrt(1/4pi), sqrt(3/4pi), sqrt(3/4pi)/2, 3 sqrt(5/12pi), (3/2) sqrt(5/12pi)
constexpr float SS_A0 = 0.28209479177387814f, SS_A1 = 0.4886025119029199f, SS_A2 = 0.24430125595145996f,
                SS_A3 = 1.0925484305920792f, SS_A4 = 0.5462742152960396f;

__host__ __device__ __forceinline__ int ss_parts(long items) { return set_parts(items, SS_BLOCK, SS_MAX_PARTS); }

__device__ __forceinline__ void ss_basis(const float* n, float* H) {
    const float nx = n[0], ny = n[1], nz = n[2];
    H[0] = SS_A0;
    H[1] = SS_A1 * nx;
    H[2] = SS_A1 * ny;
    H[3] = SS_A1 * nz;
    H[4] = SS_A2 * ((2.f * (nz * nz) - nx * nx) - ny * ny);
    H[5] = SS_A3 * (ny * nz);
    H[6] = SS_A3 * (nx * nz);
    H[7] = SS_A3 * (nx * ny);
    H[8] = SS_A4 * (nx * nx - ny * ny);
}

// sum_j sh[j] H[j], j ascending from the first product
__device__ __forceinline__ float ss_light(const float* __restrict__ sh, const float* H) {
    float L = sh[0] * H[0];
#pragma unroll
    for (int j = 1; j < 9; j++) L += sh[j] * H[j];
    return L;
}

// d[c] = sum_j sh[j] dH_j/dn_c, j ascending over the terms that depend on n_c
__device__ __forceinline__ void ss_light_gradient(const float* __restrict__ sh, const float* n, float* d) {
    const float nx = n[0], ny = n[1], nz = n[2];
    d[0] = (((sh[1] * SS_A1 + sh[4] * (SS_A2 * (-2.f * nx))) + sh[6] * (SS_A3 * nz)) + sh[7] * (SS_A3 * ny)) +
           sh[8] * (SS_A4 * (2.f * nx));
    d[1] = (((sh[2] * SS_A1 + sh[4] * (SS_A2 * (-2.f * ny))) + sh[5] * (SS_A3 * nz)) + sh[7] * (SS_A3 * nx)) +
           sh[8] * (SS_A4 * (-2.f * ny));
    d[2] = ((sh[3] * SS_A1 + sh[4] * (SS_A2 * (4.f * nz))) + sh[5] * (SS_A3 * ny)) + sh[6] * (SS_A3 * nx);
}

__device__ __forceinline__ void ss_cross(const float* a, const float* b, float* o) {
    o[0] = a[1] * b[2] - a[2] * b[1];
    o[1] = a[2] * b[0] - a[0] * b[2];
    o[2] = a[0] * b[1] - a[1] * b[0];
}

// the edges a = x1 - x0 and b = x2 - x0 of face f
__device__ __forceinline__ void ss_edges(const float* __restrict__ x, const int32_t* __restrict__ tri, long f, float* a,
                                         float* b) {
    const float* x0 = x + (size_t)tri[f * 3 + 0] * 3;
    const float* x1 = x + (size_t)tri[f * 3 + 1] * 3;
    const float* x2 = x + (size_t)tri[f * 3 + 2] * 3;
#pragma unroll
    for (int k = 0; k < 3; k++) { a[k] = x1[k] - x0[k]; b[k] = x2[k] - x0[k]; }
}

// grid (blocks of F, vb): one lane per (set, face).  face_normals [vb, F, 3].
__global__ void __launch_bounds__(SS_BLOCK) k_smooth_shade_face_normals(const float* __restrict__ vertices,
                                                                        const int32_t* __restrict__ tri,
                                                                        float* __restrict__ face_normals, int V, long F) {
    const long f = (long)blockIdx.x * SS_BLOCK + threadIdx.x;
    if (f >= F) return;
    const int b = blockIdx.y;
    float ea[3], eb[3], n[3];
    ss_edges(vertices + (size_t)b * V * 3, tri, f, ea, eb);
    ss_cross(ea, eb, n);
    float* o = face_normals + ((size_t)b * F + f) * 3;
    o[0] = n[0]; o[1] = n[1]; o[2] = n[2];
}

// grid (n_chunks, vb): the chunk sums of the long rows.  Item e's term is the three floats at src[b, items[e] / DIV]:
// DIV = 3 reads a face's normal (src [vb, F, 3]), DIV = 1 an item's own term (src [vb, 3 F, 3]).  partials [vb, n_chunks, 3].
template <int DIV>
__global__ void __launch_bounds__(RG_BLOCK) k_smooth_shade_chunks(const int32_t* __restrict__ adj_items,
                                                                  const int2* __restrict__ chunks, int n_chunks,
                                                                  const float* __restrict__ src, long per_set,
                                                                  float* __restrict__ partials) {
    const int ch = blockIdx.x, b = blockIdx.y;
    const float* s = src + (size_t)b * per_set * 3;
    float sum[3];
    rg_chunk_sum(chunks[ch], sum, [&](int e, float (&acc)[3]) {
        const float* t = s + (size_t)(adj_items[e] / DIV) * 3;
#pragma unroll
        for (int k = 0; k < 3; k++) acc[k] += t[k];
    });
    if (threadIdx.x == 0) {
        float* out = partials + ((size_t)b * n_chunks + ch) * 3;
        out[0] = sum[0]; out[1] = sum[1]; out[2] = sum[2];
    }
}

// grid (blocks of V, vb): one lane per (vertex set, vertex) walks its row, normalises, stores normals [vb, V, 3] and lengths
// [vb, V]; with colours it evaluates the basis once and shades its set (vb > 1) or every set in ascending order (shared
// vertices): shaded [B, V, 3].
__global__ void __launch_bounds__(SS_BLOCK) k_smooth_shade_vertices(CsrRows adj, const float* __restrict__ face_normals,
                                                                    const float* __restrict__ partials,
                                                                    const float* __restrict__ colors, int cb,
                                                                    const float* __restrict__ sh, int sb,
                                                                    float* __restrict__ shaded, float* __restrict__ normals,
                                                                    float* __restrict__ lengths, int B, int vb, int V,
                                                                    long F) {
    const int v = blockIdx.x * SS_BLOCK + threadIdx.x;
    if (v >= V) return;
    const int bv = blockIdx.y;
    const int start = adj.offsets[v], end = adj.offsets[v + 1];
    float s[3] = {0.f, 0.f, 0.f};
    if (rg_is_long(adj.longs, end - start)) {
        rg_add_chunk_sums<3>(adj.longs, rg_find_long(adj.longs, v), partials + (size_t)bv * adj.longs.n_chunks * 3, s);
    } else {
        const float* nf = face_normals + (size_t)bv * F * 3;
        for (int e = start; e < end; e++) {
            const float* t = nf + (size_t)(adj.items[e] / 3) * 3;
            s[0] += t[0]; s[1] += t[1]; s[2] += t[2];
        }
    }
    const float r = sqrtf((s[0] * s[0] + s[1] * s[1]) + s[2] * s[2]);
    const float d = fmaxf(r, SS_EPS);
    const float n[3] = {s[0] / d, s[1] / d, s[2] / d};
    const size_t at = (size_t)bv * V + v;
    normals[at * 3] = n[0]; normals[at * 3 + 1] = n[1]; normals[at * 3 + 2] = n[2];
    lengths[at] = r;
    if (!colors) return;
    float H[9];
    ss_basis(n, H);
    const int b_begin = vb > 1 ? bv : 0, b_end = vb > 1 ? bv + 1 : B;
    for (int b = b_begin; b < b_end; b++) {
        const float* shp = sh + (size_t)(sb > 1 ? b : 0) * SS_SUMS;
        const float* col = colors + ((size_t)(cb > 1 ? b : 0) * V + v) * 3;
        float* o = shaded + ((size_t)b * V + v) * 3;
#pragma unroll
        for (int k = 0; k < 3; k++) o[k] = col[k] * ss_light(shp + 9 * k, H);
    }
}

// The per-vertex backward stage.  grid (parts, B), or (parts, 1) when B > 1 and the vertices or the colours are shared:
// there the workgroup walks the sets in ascending order and adds into its own elements of g_colors / g_s.
// g_shaded [B, V, 3] or NULL (zeros; then g_colors and sh_partial are NULL too); g_normals [vb, V, 3] or NULL;
// g_colors [cb, V, 3], g_s [vb, V, 3], sh_partial [B, parts, 27]: each may be NULL (not needed).
__global__ void __launch_bounds__(SS_BLOCK) k_smooth_shade_backward_vertices(const float* __restrict__ colors, int cb,
                                                                             const float* __restrict__ sh, int sb,
                                                                             const float* __restrict__ normals,
                                                                             const float* __restrict__ lengths, int vb,
                                                                             const float* __restrict__ g_shaded,
                                                                             const float* __restrict__ g_normals,
                                                                             float* g_colors, float* g_s,
                                                                             float* __restrict__ sh_partial, int B, int V,
                                                                             int walk_sets) {
    __shared__ float s_wave[2][SS_BLOCK / 64][SS_SUMS];
    const int t = threadIdx.x, parts = gridDim.x;
    const int b_begin = walk_sets ? 0 : blockIdx.y, b_end = walk_sets ? B : b_begin + 1;
    for (int b = b_begin; b < b_end; b++) {
        const float* shp = sh ? sh + (size_t)(sb > 1 ? b : 0) * SS_SUMS : nullptr;
        const int bv = vb > 1 ? b : 0, bc = cb > 1 ? b : 0;
        const bool first_v = vb > 1 || b == b_begin, last_v = vb > 1 || b == b_end - 1;
        float acc[SS_SUMS];
#pragma unroll
        for (int j = 0; j < SS_SUMS; j++) acc[j] = 0.f;
        for (int i = blockIdx.x * SS_BLOCK + t; i < V; i += parts * SS_BLOCK) {
            const size_t nat = ((size_t)bv * V + i) * 3;
            const float n[3] = {normals[nat], normals[nat + 1], normals[nat + 2]};
            float gn[3] = {0.f, 0.f, 0.f};
            if (g_shaded) {
                float H[9];
                ss_basis(n, H);
                const float* g = g_shaded + ((size_t)b * V + i) * 3;
                const size_t cat = ((size_t)bc * V + i) * 3;
#pragma unroll
                for (int k = 0; k < 3; k++) {
                    const float gk = g[k], gL = gk * colors[cat + k];
                    if (g_colors) {
                        const float gc = gk * ss_light(shp + 9 * k, H);
                        g_colors[cat + k] = (cb > 1 || b == b_begin) ? gc : g_colors[cat + k] + gc;     // (this lane's own element)
                    }
                    if (sh_partial) {
#pragma unroll
                        for (int j = 0; j < 9; j++) acc[9 * k + j] += gL * H[j];
                    }
                    if (g_s) {
                        float d[3];
                        ss_light_gradient(shp + 9 * k, n, d);
                        gn[0] += gL * d[0]; gn[1] += gL * d[1]; gn[2] += gL * d[2];
                    }
                }
            }
            if (g_s) {
                if (g_normals && first_v) { gn[0] += g_normals[nat]; gn[1] += g_normals[nat + 1]; gn[2] += g_normals[nat + 2]; }
                if (!first_v) { gn[0] = g_s[nat] + gn[0]; gn[1] = g_s[nat + 1] + gn[1]; gn[2] = g_s[nat + 2] + gn[2]; }
                if (last_v) {
                    const float r = lengths[(size_t)bv * V + i];
                    if (r >= SS_EPS) {
                        const float dot = (n[0] * gn[0] + n[1] * gn[1]) + n[2] * gn[2];
#pragma unroll
                        for (int k = 0; k < 3; k++) gn[k] = (gn[k] - n[k] * dot) / r;
                    } else {
#pragma unroll
                        for (int k = 0; k < 3; k++) gn[k] = gn[k] / SS_EPS;
                    }
                }
                g_s[nat] = gn[0]; g_s[nat + 1] = gn[1]; g_s[nat + 2] = gn[2];
            }
        }
        if (sh_partial)                                     // (uniform: the barrier is met by every lane)
            set_store_partial<SS_SUMS, WaveTree::DppRows>(    // two buffers: the next set is written while this one is read
                acc, s_wave[(b - b_begin) & 1], sh_partial, b, parts);
    }
}

// One lane per element of g_sh [sb, 3, 9]: a set's partials in ascending part order; a shared sh adds the sets' sums in
// ascending set order.
__global__ void __launch_bounds__(SS_BLOCK) k_smooth_shade_backward_finish(const float* __restrict__ sh_partial, int parts,
                                                                           float* __restrict__ g_sh, int sb, int B) {
    const int i = blockIdx.x * SS_BLOCK + threadIdx.x;
    if (i >= sb * SS_SUMS) return;
    const int q = i % SS_SUMS;
    const int b_begin = sb > 1 ? i / SS_SUMS : 0, b_end = sb > 1 ? b_begin + 1 : B;
    float total = 0.f;
    for (int b = b_begin; b < b_end; b++) {
        float s[1];
        set_add_parts<1, SS_SUMS>(sh_partial + q, b, parts, s);
        total = b == b_begin ? s[0] : total + s[0];
    }
    g_sh[i] = total;
}

// grid (blocks of F, vb): one lane per (set, face) gathers g_s at its corners and stores the three corners' terms:
// terms [vb, F, 3 corners, 3] -- item 3 f + c's term is the three floats at terms[b, 3 f + c].
__global__ void __launch_bounds__(SS_BLOCK) k_smooth_shade_backward_faces(const float* __restrict__ vertices,
                                                                          const int32_t* __restrict__ tri,
                                                                          const float* __restrict__ g_s,
                                                                          float* __restrict__ terms, int V, long F) {
    const long f = (long)blockIdx.x * SS_BLOCK + threadIdx.x;
    if (f >= F) return;
    const int b = blockIdx.y;
    const float* gs = g_s + (size_t)b * V * 3;
    const float* g0 = gs + (size_t)tri[f * 3 + 0] * 3;
    const float* g1 = gs + (size_t)tri[f * 3 + 1] * 3;
    const float* g2 = gs + (size_t)tri[f * 3 + 2] * 3;
    const float gN[3] = {(g0[0] + g1[0]) + g2[0], (g0[1] + g1[1]) + g2[1], (g0[2] + g1[2]) + g2[2]};
    float ea[3], eb[3], t1[3], t2[3];
    ss_edges(vertices + (size_t)b * V * 3, tri, f, ea, eb);
    ss_cross(eb, gN, t1);
    ss_cross(gN, ea, t2);
    float* o = terms + ((size_t)b * F + f) * 9;
#pragma unroll
    for (int k = 0; k < 3; k++) { o[k] = -(t1[k] + t2[k]); o[3 + k] = t1[k]; o[6 + k] = t2[k]; }
}

// grid (blocks of 3 V, vb): one lane per element of g_x [vb, V, 3].  A vertex of no face gets 0: every element is written.
__global__ void __launch_bounds__(SS_BLOCK) k_smooth_shade_backward_rows(CsrRows adj, const float* __restrict__ terms,
                                                                         const float* __restrict__ partials,
                                                                         float* __restrict__ g_x, int V, long F) {
    const long i = (long)blockIdx.x * SS_BLOCK + threadIdx.x;
    if (i >= (long)V * 3) return;
    const int b = blockIdx.y;
    const int v = (int)(i / 3), k = (int)(i - (long)v * 3);
    const int start = adj.offsets[v], end = adj.offsets[v + 1];
    float acc[1] = {0.f};
    if (rg_is_long(adj.longs, end - start)) {
        rg_add_chunk_sums<1, 3>(adj.longs, rg_find_long(adj.longs, v), partials + (size_t)b * adj.longs.n_chunks * 3 + k, acc);
    } else {
        const float* tm = terms + (size_t)b * F * 9 + k;
        for (int e = start; e < end; e++) acc[0] += tm[(size_t)adj.items[e] * 3];
    }
    g_x[(size_t)b * V * 3 + i] = acc[0];
}

}  // namespace d3m
