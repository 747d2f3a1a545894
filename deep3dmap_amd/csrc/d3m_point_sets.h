// d3m_point_sets.h -- nearest points and chamfer distances between point sets (neural_renderer/point_sets.py,
// core/mesh_eval.py): the data term of a fit of a mesh to a 3D target, beside d3m_mesh_reg.h's priors.  Exact brute force.
//
// NEAREST NEIGHBOUR.  Queries a [B, N, 3] and targets b [B, M, 3], f32; lengths_a [B], lengths_b [B] (int32 in device memory, or
// NULL: N and M) give the ragged sizes n_b = clamp(lengths_a[b], 0, N) and m_b likewise.  For query i < n_b and target j < m_b
//   d2(i, j) = fma(dz, dz, fma(dy, dy, dx dx)),  dx = a.x - b.x, dy = a.y - b.y, dz = a.z - b.z     (f32; never |a|^2 + |b|^2 - 2 a.b)
// and the winner is the j that minimises the pair (bits of d2, j) lexicographically: the lowest index among equal f32
// distances (the rule of d3m_bid.h).  d2 >= +0, so its bits order as the values do, with +Inf a candidate like any other; a NaN d2
// is no candidate.  Outputs index [B, N] (int32) and dist2 [B, N] (f32), every element WRITTEN:
//   i >= n_b, or m_b == 0:              index -1, dist2 +0
//   every d2(i, .) is NaN:              index -1, dist2 NaN
//   otherwise:                          the winner and its d2
//
// k_pset_nearest: a lane keeps PSET_Q queries in registers (lane t of query block q: the queries PSET_BLOCK_QUERIES q + 256 k + t,
// k < PSET_Q); the workgroup stages PSET_TILE targets in LDS as float4 (16 bytes a point) and every lane reads the same address -- a
// broadcast, no bank conflict --, one read serving the lane's PSET_Q queries.  The targets' tiles are split over `splits`
// workgroups per query block (the host's choice from the shapes alone: pset_auto_splits; split s takes the tiles
// s tiles_per_split ..), for few queries against many targets.  A lane's winner goes into the query's key
//   (bits(d2) << 32) | j          with a 64-bit INTEGER atomic min at agent scope (keys start as all ones: k_pset_init)
// so neither arrival order nor split count can change a bit.  Both directions of a chamfer distance run in the same launches.
//
// VALUE.  Per batch element b and direction (a -> b shown):  L_ab = (1 / n_b) sum_{i < n_b} rho(d2_i),  rho(d2) = d2 (squared) or
// sqrt(d2); with truncation tau a term with d2 > tau^2 contributes rho(tau^2) (f32 tau tau) and has no gradient; at equality it is
// not truncated.  value[b] = weight_ab L_ab + weight_ba L_ba over the directions of weight > 0, in this order (a direction of
// weight 0 is not evaluated); a direction whose query set is empty (or whose target set is: every dist2 is +0) adds +0.  The sum
// over a set runs in the tree of d3m_set_sums.h (a set is a batch element, an element a point; PSET_PER_PART points per part, at
// most PSET_MAX_PARTS parts, DppRows), L = S / (float)n_b, and coef[b][dir] = weight / n_b (formed in f64, rounded once; 0 for an
// empty query set or a direction that is off) is left for the backward.
//
// ADJOINT.  The argmin is a constant.  Point i of a set in its role as QUERY receives the direct term
//   t_i = (s_i (q_i - t_nn(i))) + 0,   s_i = (upstream[b] coef[b][dir]) rho'(d2_i);   rho' = 2 (squared), 1 / sqrt(d2) (exactly 0 at
//   d2 == 0) otherwise; with per-query upstream gradients of dist2 (nearest_points): s_i = 2 upstream[b, i]
// a plain store, every element written: truncated terms, points beyond the set's length, points of an empty target set and a
// direction that is off get exactly +0; a point whose index is -1 because every d2 was NaN gets NaN.  In its role as somebody's
// NEAREST NEIGHBOUR a point receives minus those terms: a scatter whose destinations change every step, done as
// d3m_uv_texture.h does its own (lines 20-36; uvt_block_max, uvt_gmax_bits, uvt_quantum are used as they stand):
//   gmax     max |t_i| over the call's direct terms of both directions, on the bits of |x| (per-workgroup maxima, plain stores)
//   quantum  E = ilogb(gmax) + 1, frac = 62 - ceil(log2(max(N, M))) (the host passes it)
//   add      __double2ll_rn((double)(-t) 2^(frac - E)) with a 64-bit integer atomic add into one int64 accumulator per coordinate
//            of every point of both sets, cleared by k_pset_direct itself; a coordinate of exactly 0 adds nothing
//   result   grad = direct + (float)((double)acc 2^(E - frac)), in this order
// |t| <= gmax < 2^E and at most max(N, M) terms reach one point, so |sum| <= 2^62: no overflow.  gmax == 0: every element of both
// gradients is an exact +0.  gmax not finite: every element is NaN.  Nothing goes back to the host; no float atomics.
//
// LAUNCHES, whatever B, N, M, the lengths and the options:
//   nearest points    3: k_pset_init, k_pset_nearest, k_pset_resolve
//   chamfer forward   4: k_pset_init, k_pset_nearest, k_pset_resolve, k_pset_value_finish
//   backward          3: k_pset_direct, k_pset_scatter, k_pset_convert
#pragma once
#include "d3m_set_sums.h"
#include "d3m_uv_texture.h"

namespace d3m {

constexpr int PSET_Q = 4;                         // queries a lane keeps in registers
constexpr int PSET_TILE = 512;                    // targets staged in LDS at a time (8 KB)
constexpr int PSET_BLOCK_QUERIES = 256 * PSET_Q;    // queries of a workgroup
constexpr int PSET_PER_PART = 4 * SET_BLOCK;      // points per part of a set's value sum
constexpr int PSET_MAX_PARTS = 256;
constexpr int PSET_MAX_POINTS = 1 << 30;          // N, M
constexpr int PSET_FILL_BLOCKS = 1024;            // the fixed grids of k_pset_init and of the three adjoint kernels: their block maxima
constexpr int PSET_TARGET_WORKGROUPS = 1024;      // pset_auto_splits fills the chip to about this many workgroups
constexpr unsigned long long PSET_NO_KEY = ~0ull;
constexpr uint32_t PSET_NO_BITS = 0x7F800001u;    // above the bits of +Inf: a NaN d2 (0x7F800001 .. and the negative ones) never wins

__host__ __device__ __forceinline__ int pset_tiles(int M) { return (M + PSET_TILE - 1) / PSET_TILE; }
__host__ __device__ __forceinline__ int pset_query_blocks(int N) { return (N + PSET_BLOCK_QUERIES - 1) / PSET_BLOCK_QUERIES; }
__host__ __device__ __forceinline__ int pset_parts(int N) { return set_parts(N, PSET_PER_PART, PSET_MAX_PARTS); }

// the split count of one direction: a function of the shapes only
inline int pset_auto_splits(int B, int N, int M) {
    const long groups = (long)B * pset_query_blocks(N);
    long want = (PSET_TARGET_WORKGROUPS + groups - 1) / groups;
    const int tiles = pset_tiles(M);
    if (want > tiles) want = tiles;
    return want < 1 ? 1 : (int)want;
}

__device__ __forceinline__ int pset_length(const int* __restrict__ lengths, int b, int full) {
    if (!lengths) return full;
    const int n = lengths[b];
    return n < 0 ? 0 : (n > full ? full : n);
}

// one direction of a search: queries q [B, N, 3] against targets t [B, M, 3]
struct PsetDir {
    const float* q;
    const float* t;
    const int* len_q;
    const int* len_t;
    unsigned long long* keys;       // [B, N]
    int* index;                     // [B, N]
    float* dist2;                   // [B, N]
    float* partial;                 // [B, parts] or NULL (no value)
    int N, M, splits, tiles_per_split, parts;
    int on;                         // 0: the direction is not evaluated and nothing of it is read or written
};
struct PsetSearch {
    PsetDir ab, ba;                   // a -> b; b -> a
    int B;
};
// (a direction is picked by a wave-uniform select between the two members, never by indexing an array of them with a run-time
//  index: that would move the kernel's arguments to scratch)
__device__ __forceinline__ PsetDir pset_dir(const PsetSearch& s, unsigned which) { return which ? s.ba : s.ab; }

// ---- 1. the keys start as "nothing" ----------------------------------------------------------------------------------------------
__device__ __forceinline__ void pset_init_keys(const PsetDir& d, int B) {
    if (!d.on) return;
    const size_t n = (size_t)B * d.N;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) d.keys[i] = PSET_NO_KEY;
}
__global__ void __launch_bounds__(256) k_pset_init(PsetSearch s) {
    pset_init_keys(s.ab, s.B);
    pset_init_keys(s.ba, s.B);
}

// ---- 2. the search: grid (max over the directions of query blocks x splits, B, 2 or 1) ----------------------------------------------
__global__ void __launch_bounds__(256) k_pset_nearest(PsetSearch s) {
    __shared__ float4 s_t[PSET_TILE];
    const PsetDir d = pset_dir(s, blockIdx.z);
    if (!d.on) return;
    const int b = blockIdx.y;
    const unsigned qb = blockIdx.x / (unsigned)d.splits, sp = blockIdx.x - qb * (unsigned)d.splits;
    const int n = pset_length(d.len_q, b, d.N), m = pset_length(d.len_t, b, d.M);
    // (uniform over the workgroup: no lane is left behind at a barrier)
    if ((long)qb * PSET_BLOCK_QUERIES >= n) return;                       // also the surplus workgroups of the smaller direction
    const int t0 = (int)sp * d.tiles_per_split, t1 = min(t0 + d.tiles_per_split, pset_tiles(m));
    if (t0 >= t1) return;
    const float* q = d.q + (size_t)b * d.N * 3;
    const float* t = d.t + (size_t)b * d.M * 3;
    const int i0 = (int)qb * PSET_BLOCK_QUERIES + (int)threadIdx.x;
    float x[PSET_Q], y[PSET_Q], z[PSET_Q];
    uint32_t best[PSET_Q];
    int best_j[PSET_Q];
#pragma unroll
    for (int k = 0; k < PSET_Q; k++) {
        const int i = i0 + k * 256;
        const bool on = i < n;
        x[k] = on ? q[(size_t)i * 3] : 0.f;
        y[k] = on ? q[(size_t)i * 3 + 1] : 0.f;
        z[k] = on ? q[(size_t)i * 3 + 2] : 0.f;
        best[k] = PSET_NO_BITS;
        best_j[k] = -1;
    }
    for (int tile = t0; tile < t1; tile++) {
        const int j0 = tile * PSET_TILE, cnt = min(PSET_TILE, m - j0);
        __syncthreads();                                                // the last tile has been read
        for (int e = threadIdx.x; e < cnt; e += 256) {
            const float* p = t + (size_t)(j0 + e) * 3;
            s_t[e] = make_float4(p[0], p[1], p[2], 0.f);
        }
        __syncthreads();
#pragma unroll 4
        for (int e = 0; e < cnt; e++) {
            const float4 p = s_t[e];
#pragma unroll
            for (int k = 0; k < PSET_Q; k++) {
                const float dx = x[k] - p.x, dy = y[k] - p.y, dz = z[k] - p.z;
                const uint32_t bits = __float_as_uint(fmaf(dz, dz, fmaf(dy, dy, dx * dx)));
                const bool wins = bits < best[k];                       // strict: the lowest index among equals stays
                best[k] = wins ? bits : best[k];
                best_j[k] = wins ? j0 + e : best_j[k];
            }
        }
    }
#pragma unroll
    for (int k = 0; k < PSET_Q; k++) {
        const int i = i0 + k * 256;
        if (i < n && best_j[k] >= 0) {
            const unsigned long long key = ((unsigned long long)best[k] << 32) | (uint32_t)best_j[k];
            __hip_atomic_fetch_min(d.keys + (size_t)b * d.N + i, key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
}

// rho of a distance that counts, truncated at tau2 (< 0: not truncated); a NaN stays a NaN
__device__ __forceinline__ float pset_rho(float d2, bool squared, float tau2) {
    const float v = (tau2 >= 0.f && d2 > tau2) ? tau2 : d2;
    return squared ? v : sqrtf(v);
}

// ---- 3. keys -> index and dist2, and the parts of the value's sums: grid (max parts, B, 2 or 1) ---------------------------------------
__global__ void __launch_bounds__(SET_BLOCK) k_pset_resolve(PsetSearch s, int squared, float tau2) {
    __shared__ float s_wave[4][1];
    const PsetDir d = pset_dir(s, blockIdx.z);
    const int b = blockIdx.y, parts = d.parts;
    if (!d.on || (int)blockIdx.x >= parts) return;                      // (uniform)
    const int n = pset_length(d.len_q, b, d.N), m = pset_length(d.len_t, b, d.M);
    const unsigned long long* keys = d.keys + (size_t)b * d.N;
    int* index = d.index + (size_t)b * d.N;
    float* dist2 = d.dist2 + (size_t)b * d.N;
    float acc[1] = {0.f};
    for (int i = blockIdx.x * SET_BLOCK + threadIdx.x; i < d.N; i += parts * SET_BLOCK) {
        int j = -1;
        float d2 = 0.f;
        if (i < n && m > 0) {
            const unsigned long long key = keys[i];
            if (key == PSET_NO_KEY) d2 = __uint_as_float(0x7FC00000u);
            else {
                j = (int)(uint32_t)key;
                d2 = __uint_as_float((uint32_t)(key >> 32));
            }
            acc[0] += pset_rho(d2, squared != 0, tau2);
        }
        index[i] = j;
        dist2[i] = d2;
    }
    if (d.partial) set_store_partial<1, WaveTree::DppRows>(acc, s_wave, d.partial, b, parts);      // (uniform)
}

// ---- 4. value [B] and coef [B, 2]: a workgroup per batch element stages the parts, lane 0 adds them in ascending order ------------------
__device__ __forceinline__ void pset_stage_parts(const PsetDir& d, int b, float* staged) {
    if (!d.on) return;
    for (int i = threadIdx.x; i < d.parts; i += SET_BLOCK) staged[i] = d.partial[(size_t)b * d.parts + i];
}
// weight L of one direction, its coefficient left in c; +0 and 0 for an empty query set
__device__ __forceinline__ float pset_direction_term(const PsetDir& d, int b, float weight, const float* staged, float& c) {
    const int n = pset_length(d.len_q, b, d.N);
    float sum[1];
    set_add_parts<1>(staged, 0, d.parts, sum);
    c = n > 0 ? (float)((double)weight / (double)n) : 0.f;
    return n > 0 ? weight * (sum[0] / (float)n) : 0.f;
}
__global__ void __launch_bounds__(SET_BLOCK) k_pset_value_finish(PsetSearch s, float weight_ab, float weight_ba, float* __restrict__ coef,
                                                               float* __restrict__ value) {
    __shared__ float s_part[2][PSET_MAX_PARTS];
    const int b = blockIdx.x;
    pset_stage_parts(s.ab, b, s_part[0]);
    pset_stage_parts(s.ba, b, s_part[1]);
    __syncthreads();
    if (threadIdx.x != 0) return;
    float c_ab = 0.f, c_ba = 0.f, total = 0.f;
    if (s.ab.on) total = pset_direction_term(s.ab, b, weight_ab, s_part[0], c_ab);
    if (s.ba.on) {
        const float term = pset_direction_term(s.ba, b, weight_ba, s_part[1], c_ba);
        total = s.ab.on ? total + term : term;
    }
    value[b] = total;
    coef[2 * b] = c_ab;
    coef[2 * b + 1] = c_ba;
}

// ---- the adjoint -----------------------------------------------------------------------------------------------------------------------
// one direction as the adjoint reads it; off (index == NULL): its queries' direct terms are +0 and nothing is scattered
struct PsetAdjDir {
    const float* q;                 // [B, N, 3]
    const float* t;                 // [B, M, 3]
    const int* len_q;
    const int* len_t;
    const int* index;               // [B, N] or NULL
    const float* dist2;             // [B, N]
    float* grad_q;                  // [B, N, 3]: the direct terms, then the gradient
    long long* acc_q;               // [B, N, 3]: the accumulators of this direction's QUERIES: what the other direction scatters
    long long* acc_t;               // [B, M, 3]: those of its targets: the other direction's acc_q
    int N, M, dir;                  // dir: 0 a -> b, 1 b -> a (the column of coef)
};
struct PsetAdjoint {
    PsetAdjDir ab, ba;
    const float* coef;              // [B, 2] or NULL (per-query upstream)
    const float* upstream;          // [B], or [B, N] with per_query
    int B, per_query, squared;
    float tau2;
};

// 1. every point's direct term, stored; its three accumulators cleared; the lane's max of the bits of |term| (one direction)
__device__ __forceinline__ unsigned pset_direct_terms(const PsetAdjoint& a, const PsetAdjDir& d) {
    const long total = (long)a.B * d.N;
    unsigned v = 0;
    for (long p = (long)blockIdx.x * 256 + threadIdx.x; p < total; p += (long)gridDim.x * 256) {
        const int b = (int)(p / d.N), i = (int)(p - (long)b * d.N);
        float g[3] = {0.f, 0.f, 0.f};
        if (d.index && i < pset_length(d.len_q, b, d.N) && pset_length(d.len_t, b, d.M) > 0) {
            const int j = d.index[p];
            const float d2 = d.dist2[p];
            if (j < 0) {                                                // every candidate's d2 was NaN
                g[0] = g[1] = g[2] = __uint_as_float(0x7FC00000u);
            } else {
                float slope;
                bool cut = false;
                if (a.per_query) slope = 2.f * a.upstream[p];
                else {
                    const float c = a.upstream[b] * a.coef[2 * b + d.dir];
                    cut = a.tau2 >= 0.f && d2 > a.tau2;
                    slope = c * (a.squared ? 2.f : (d2 > 0.f ? 1.f / sqrtf(d2) : 0.f));
                }
                if (!cut) {
                    const float* qp = d.q + (size_t)p * 3;
                    const float* tp = d.t + ((size_t)b * d.M + j) * 3;
#pragma unroll
                    for (int k = 0; k < 3; k++) g[k] = slope * (qp[k] - tp[k]) + 0.f;      // (-0 + +0 is +0)
                }
            }
        }
#pragma unroll
        for (int k = 0; k < 3; k++) {
            d.grad_q[(size_t)p * 3 + k] = g[k];
            d.acc_q[(size_t)p * 3 + k] = 0;
            v = max(v, __float_as_uint(g[k]) & 0x7FFFFFFFu);
        }
    }
    return v;
}
__global__ void __launch_bounds__(256) k_pset_direct(PsetAdjoint a, unsigned* __restrict__ block_max) {
    unsigned v = max(pset_direct_terms(a, a.ab), pset_direct_terms(a, a.ba));
    v = uvt_block_max(v);
    if (threadIdx.x == 0) block_max[blockIdx.x] = v;
}

// 2. minus every direct term, quantised, added to the accumulators of the term's nearest neighbour
__device__ __forceinline__ void pset_scatter_terms(const PsetAdjoint& a, const PsetAdjDir& d, const UvtQuantum& qn) {
    if (!d.index) return;
    const long total = (long)a.B * d.N;
    for (long p = (long)blockIdx.x * 256 + threadIdx.x; p < total; p += (long)gridDim.x * 256) {
        const int j = d.index[p];
        if (j < 0) continue;
        const int b = (int)(p / d.N);
        unsigned long long* dst = (unsigned long long*)d.acc_t + ((size_t)b * d.M + j) * 3;
#pragma unroll
        for (int k = 0; k < 3; k++) {
            const float term = d.grad_q[(size_t)p * 3 + k];
            if (term == 0.f) continue;
            const long long fixed = __double2ll_rn(-(double)term * qn.up);
            __hip_atomic_fetch_add(dst + k, (unsigned long long)fixed, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
}
__global__ void __launch_bounds__(256) k_pset_scatter(PsetAdjoint a, const unsigned* __restrict__ block_max, int n_max, int frac) {
    const UvtQuantum qn = uvt_quantum(uvt_gmax_bits(block_max, n_max), frac);
    if (qn.state != UVT_FINITE) return;
    pset_scatter_terms(a, a.ab, qn);
    pset_scatter_terms(a, a.ba, qn);
}

// 3. grad = direct + scattered, every element of both gradients written
__device__ __forceinline__ void pset_convert_terms(const PsetAdjoint& a, const PsetAdjDir& d, const UvtQuantum& qn) {
    const long total = (long)a.B * d.N * 3;
    for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long)gridDim.x * 256) {
        float v = 0.f;
        if (qn.state == UVT_FINITE) v = d.grad_q[e] + (float)((double)d.acc_q[e] * qn.down);
        else if (qn.state == UVT_NOT_FINITE) v = __uint_as_float(0x7FC00000u);
        d.grad_q[e] = v;
    }
}
__global__ void __launch_bounds__(256) k_pset_convert(PsetAdjoint a, const unsigned* __restrict__ block_max, int n_max, int frac) {
    const UvtQuantum qn = uvt_quantum(uvt_gmax_bits(block_max, n_max), frac);
    pset_convert_terms(a, a.ab, qn);
    pset_convert_terms(a, a.ba, qn);
}

}  // namespace d3m
